// drive_select.cpp — drives fmhip_compress, fmhip_expand and fmhip_gather through the C-ABI on the TEST-ONLY null device under the
// sanitizers.  The vectors hold real data and the stand-ins of null_select.cpp walk the chunks and the tiles the kernels' way, so results
// are CHECKED against the definitions (the _host twins): every mask family, 0, 1 and 8 value vectors, positions on and off, the count
// alone, at n = 1, 65, one tile + 1, the smallest n with two and with three chunks and 300 007 (scratch and stage grow between the calls),
// and 65 and 1 again behind the large one; count == 0 (every handle 0, the pool as it was); the size mismatch of an expand, found after
// the count; hostile indices; pending operands; every argument error that is found on the host.  Twice, with a shutdown and a
// re-initialisation in between; then once more behind a device list of ONE shard.  FMNULL_DEVICES=N: behind N shards every call is
// FMHIP_ERR_UNSUPPORTED and leaves nothing behind; FMNULL_THREAD_ENGINES=1: the calls come from a thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one compress and one expand in which a pool allocation fails — BETWEEN the
// two phases, where the outputs are allocated.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"
#include "../../finmath-lib-cuda-extensions_amd/csrc/select_host.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(const F& a, const float* b, int64_t count) { return count == 0 || std::memcmp(a.data(), b, (size_t)count * 4) == 0; }

static const int FAMILIES = 9;
static F mask_of(int64_t n, int family, uint32_t seed) {
    F m((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    const float odd[6] = { std::numeric_limits<float>::quiet_NaN(), -0.f, 0.f, -1e-45f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        const float u = (float)(s >> 8) * (1.0f / 16777216.0f);
        float x;
        switch (family) {
        case 0: x = 1.f; break;
        case 1: x = -1.f; break;
        case 2: x = p == 0 ? 0.f : -1.f; break;
        case 3: x = p == n - 1 ? 2.f : -2.f; break;
        case 4: x = (p & 1) ? 1.f : -1.f; break;
        case 5: x = p % 64 == 17 % (n < 64 ? n : 64) ? 1.f : -1.f; break;
        case 6: x = u - 0.5f; break;
        case 7: x = u - 0.99f; break;
        default: x = odd[(s >> 9) % 6u];
        }
        m[(size_t)p] = x;
    }
    return m;
}
static F data(int64_t n, uint32_t seed) {          // values with NaN payloads and -0.0 among them
    F a((size_t)n);
    for (int64_t p = 0; p < n; ++p) {
        uint32_t bits = ((uint32_t)p * 2654435761u + seed) & 0x7f7fffffu;
        if (p % 7 == 1) bits = 0x7fc01234u + (uint32_t)(p & 0xff);
        if (p % 7 == 3) bits = 0x80000000u;
        std::memcpy(&a[(size_t)p], &bits, 4);
    }
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static int64_t size_of(V h) { int64_t n = -1; OK(fmhip_vec_size(h, &n)); return n; }
static fmhip_pool_stats_t pool() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st; }
static int64_t live() { return pool().n_live_vectors; }

// compress with k of the vectors, then expand what came back and gather by the positions: all against the definitions
static void check(V vm, const F& mask, const std::vector<V>& vx, const std::vector<F>& x, int k, bool want_positions, bool want_count) {
    const int64_t n = (int64_t)mask.size();
    std::vector<F> want((size_t)k, F((size_t)n));
    std::vector<int64_t> pos((size_t)n, -7);
    const float* in[8]; float* columns[8];
    for (int i = 0; i < k; ++i) { in[i] = x[(size_t)i].data(); columns[i] = want[(size_t)i].data(); }
    int64_t count_host = -1, count = -1;
    OK(fmhip_compress_host(mask.data(), n, in, k, columns, pos.data(), &count_host));
    const fmhip_pool_stats_t before = pool();
    V out[8] = { -1, -1, -1, -1, -1, -1, -1, -1 }, vp = -1;
    OK(fmhip_compress(vm, vx.data(), k, out, want_positions ? &vp : nullptr, want_count ? &count : nullptr));
    if (want_count && count != count_host) die("the count", n, count);
    if (count_host == 0) {
        const fmhip_pool_stats_t after = pool();
        for (int i = 0; i < k; ++i) if (out[i] != 0) die("a handle of an empty compress", n, i);
        if (want_positions && vp != 0) die("the positions' handle of an empty compress", n, 0);
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("an empty compress left something behind", n, 0);
        return;
    }
    for (int i = 0; i < k; ++i) {
        if (size_of(out[i]) != count_host) die("the size of a compressed vector", n, size_of(out[i]));
        if (!same(download(out[i], count_host), want[(size_t)i].data(), count_host)) die("a compressed vector", n, i);
    }
    if (want_positions) {
        const F got = download(vp, count_host);
        for (int64_t q = 0; q < count_host; ++q) if (got[(size_t)q] != (float)pos[(size_t)q]) die("the positions", n, q);
    }
    if (k > 0) {
        // expand: the inverse, with every kind of fill
        const double fills[4] = { 0.0, -0.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN() };
        const double fill = fills[(n + k) % 4];
        std::vector<F> back((size_t)k, F((size_t)n));
        const float* sin[8]; float* bout[8];
        for (int i = 0; i < k; ++i) { sin[i] = want[(size_t)i].data(); bout[i] = back[(size_t)i].data(); }
        OK(fmhip_expand_host(mask.data(), n, sin, k, count_host, fill, bout));
        V expanded[8] = { 0 };
        OK(fmhip_expand(vm, out, k, fill, expanded));
        for (int i = 0; i < k; ++i) {
            if (size_of(expanded[i]) != n || !same(download(expanded[i], n), back[(size_t)i].data(), n)) die("an expanded vector", n, i);
            rel(expanded[i]);
        }
        // gather by the positions is the compress
        if (want_positions) {
            V gathered[8] = { 0 };
            OK(fmhip_gather(vp, vx.data(), k, gathered));
            for (int i = 0; i < k; ++i) {
                if (size_of(gathered[i]) != count_host || !same(download(gathered[i], count_host), want[(size_t)i].data(), count_host)) die("a gathered vector", n, i);
                rel(gathered[i]);
            }
        }
    }
    for (int i = 0; i < k; ++i) rel(out[i]);
    if (want_positions) rel(vp);
}

static void hostile_gather(V vx, const F& x) {
    const int64_t n = (int64_t)x.size();
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    F index = { -1.f, -0.f, (float)(n - 1), (float)n, 0.5f, nan, inf, -inf, 0.f, 3e38f, -3e38f };
    for (int64_t j = 0; j < 5000; ++j) index.push_back((float)((j * 7919) % (n + 3)) - 1.f);      // more than one tile of outputs
    const int64_t m = (int64_t)index.size();
    F want((size_t)m); const float* in[1] = { x.data() }; float* columns[1] = { want.data() };
    OK(fmhip_gather_host(index.data(), m, in, 1, n, columns));
    V vi = upload(index), out = 0;
    OK(fmhip_gather(vi, &vx, 1, &out));
    if (!same(download(out, m), want.data(), m)) die("a gather by hostile indices", n, 0);
    rel(out); rel(vi);
}

static void check_all(const std::vector<V>& vx, const std::vector<F>& x, int64_t n) {
    for (int family = 0; family < FAMILIES; ++family) {
        const F mask = mask_of(n, family, (uint32_t)(n + family));
        V vm = upload(mask);
        check(vm, mask, vx, x, 1, true, true);
        check(vm, mask, vx, x, 0, false, true);
        check(vm, mask, vx, x, 0, true, false);
        check(vm, mask, vx, x, 1, false, false);
        if (family >= 5 || n < 5000) check(vm, mask, vx, x, 8, true, true);
        if (!same(download(vm, n), mask.data(), n)) die("the mask changed", n, family);
        rel(vm);
    }
    hostile_gather(vx[0], x[0]);
    if (!same(download(vx[0], n), x[0].data(), n)) die("a value vector changed", n, 0);
}

static void refusals(V vx, int64_t n) {
    const F mask = mask_of(n, 6, 5);
    std::vector<int64_t> sel;
    for (int64_t r = 0; r < n; ++r) if (mask[(size_t)r] >= 0.0f) sel.push_back(r);
    const int64_t count = (int64_t)sel.size();
    V vm = upload(mask), longer = upload(F((size_t)n + 1, 1.f)), fits = upload(F((size_t)count, 1.f)), too_long = upload(F((size_t)count + 1, 1.f));
    const fmhip_pool_stats_t before = pool();
    V out[9] = { 0 }, vp = 0; int64_t c = -7;
    V nine[9] = { vx, vx, vx, vx, vx, vx, vx, vx, vx }, with_zero[2] = { vx, 0 }, mixed[2] = { fits, too_long };
    const int bad = FMHIP_ERR_INVALID_ARGUMENT;
    EXPECT(fmhip_compress(vm, nine, 9, out, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, &vx, -1, out, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, nullptr, 0, nullptr, nullptr, nullptr), bad);                 // nothing asked for
    EXPECT(fmhip_compress(0, &vx, 1, out, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, nullptr, 1, out, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, &vx, 1, nullptr, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, with_zero, 2, out, &vp, &c), bad);
    EXPECT(fmhip_compress(vm, &longer, 1, out, &vp, &c), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_compress(vm + 12345, &vx, 1, out, &vp, &c), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_expand(vm, &fits, 0, 0.0, out), bad);
    EXPECT(fmhip_expand(vm, nine, 9, 0.0, out), bad);
    EXPECT(fmhip_expand(0, &fits, 1, 0.0, out), bad);
    EXPECT(fmhip_expand(vm, nullptr, 1, 0.0, out), bad);
    EXPECT(fmhip_expand(vm, &fits, 1, 0.0, nullptr), bad);
    EXPECT(fmhip_expand(vm, with_zero, 2, 0.0, out), bad);
    EXPECT(fmhip_expand(vm, mixed, 2, 0.0, out), FMHIP_ERR_SIZE_MISMATCH);                  // among themselves: before the count
    EXPECT(fmhip_expand(vm, &too_long, 1, 0.0, out), FMHIP_ERR_SIZE_MISMATCH);              // against the count: after it
    EXPECT(fmhip_expand(vm, &vx, 1, 0.0, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_expand(vm, &fits, 1, 0.0, out), FMHIP_OK);
    if (size_of(out[0]) != n) die("the size of an expanded vector", n, 0);
    rel(out[0]); out[0] = 0;
    EXPECT(fmhip_gather(vm, &vx, 0, out), bad);
    EXPECT(fmhip_gather(vm, nine, 9, out), bad);
    EXPECT(fmhip_gather(0, &vx, 1, out), bad);
    EXPECT(fmhip_gather(vm, nullptr, 1, out), bad);
    EXPECT(fmhip_gather(vm, &vx, 1, nullptr), bad);
    EXPECT(fmhip_gather(vm, mixed, 2, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_gather(vm, &vx + 0, 1, out + 1), FMHIP_OK);
    rel(out[1]); out[1] = 0;
    const fmhip_pool_stats_t after = pool();
    if (out[0] != 0 || vp != 0 || c != -7 || after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", n, after.n_live_vectors - before.n_live_vectors);
    rel(vm); rel(longer); rel(fits); rel(too_long);
}

static void unsupported(V vx, int64_t n) {
    const F mask = mask_of(n, 6, 5);
    V vm = upload(mask);
    const int64_t before = live();
    V out = 0, vp = 0; int64_t c = -7;
    EXPECT(fmhip_compress(vm, &vx, 1, &out, &vp, &c), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_compress(vm, nullptr, 0, nullptr, nullptr, &c), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_expand(vm, &vx, 1, 0.0, &out), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_gather(vm, &vx, 1, &out), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_compress(vm, &vx, 9, &out, &vp, &c), FMHIP_ERR_INVALID_ARGUMENT);          // the checks still come first
    EXPECT(fmhip_gather(vm, &vx, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
    if (out != 0 || vp != 0 || c != -7 || live() != before) die("a device list of several shards left something behind", n, live() - before);
    rel(vm);
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t TWO = fm::prefix_chunk_elems(1) + 1, THREE = 2 * fm::prefix_chunk_elems(1) + 1;
    if (fm::prefix_blocks(TWO) != 2 || fm::prefix_blocks(TWO - 1) != 1 || fm::prefix_blocks(THREE) != 3) die("the smallest n with two and three chunks", TWO, THREE);
    const int64_t sizes[8] = { 1, 65, fm::FM_PREFIX_TILE + 1, TWO, THREE, 300007, 65, 1 };
    for (int64_t n : sizes) {
        std::vector<F> x; std::vector<V> vx;
        for (int i = 0; i < 8; ++i) { x.push_back(data(n, (uint32_t)(n + 1 + i))); vx.push_back(upload(x.back())); }
        if (sharded) unsupported(vx[0], n);
        else {
            const int64_t before = live();
            if (thread_engines) {
                std::thread asker([&] { check_all(vx, x, n); });                         // a thread that owns none of them
                asker.join();
                if (n < 300000) check_all(vx, x, n);                                     // and the owner
            }
            else check_all(vx, x, n);
            if (n == 65 || n == THREE) refusals(vx[0], n);
            if (live() != before) die("the calls left vectors behind", n, live() - before);
        }
        for (V h : vx) rel(h);
    }
    if (sharded) return;
    // pending operands: the results against what the vectors hold once they exist
    const int64_t n = THREE;
    V stored = upload(mask_of(n, 6, 7)), state = upload(data(n, 8));
    V pending_m = 0, pending_x = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_SUB_S, stored, 0.125, &pending_m));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, state, 1.0, &pending_x));
    V out = 0, back = 0; int64_t count = -1;
    OK(fmhip_compress(pending_m, &pending_x, 1, &out, nullptr, &count));
    OK(fmhip_expand(pending_m, &out, 1, -1.0, &back));
    {
        const F m = download(pending_m, n), x = download(pending_x, n);
        F want((size_t)n), again((size_t)n); const float* in[1] = { x.data() }; float* columns[1] = { want.data() }; int64_t count_host = -1;
        OK(fmhip_compress_host(m.data(), n, in, 1, columns, nullptr, &count_host));
        const float* sin[1] = { want.data() }; float* bout[1] = { again.data() };
        OK(fmhip_expand_host(m.data(), n, sin, 1, count_host, -1.0, bout));
        if (count != count_host || !same(download(out, count), want.data(), count) || !same(download(back, n), again.data(), n)) die("a compress of pending vectors", n, 0);
    }
    rel(out); rel(back); rel(stored); rel(state); rel(pending_m); rel(pending_x);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller.  A compress with one value vector and the positions takes TWO pool allocations, both
// between its phases; the expand that follows takes ONE, between its phases too.  Without the variable this is the counting run.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 9001;
    const F mask = mask_of(n, 6, 5), x = data(n, 6);
    V vm = upload(mask), vx = upload(x);
    V fits = 0; int64_t count = 0;
    {   // what the expand will be given: made on the host, so that it costs no pool allocation inside the counted calls
        F shorter((size_t)n); const float* in[1] = { x.data() }; float* columns[1] = { shorter.data() };
        OK(fmhip_compress_host(mask.data(), n, in, 1, columns, nullptr, &count));
        shorter.resize((size_t)count);
        fits = upload(shorter);
    }
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out = 0, vp = 0, back = 0; int64_t c = -7;
        int st = fmhip_compress(vm, &vx, 1, &out, &vp, &c);
        if (st == FMHIP_OK) { rel(out); rel(vp); }
        else if (out != 0 || vp != 0 || c != -7) die("a failed compress wrote its outputs", n, 0);
        const int st2 = fmhip_expand(vm, &fits, 1, 0.0, &back);
        if (st2 == FMHIP_OK) rel(back);
        else if (back != 0) die("a failed expand wrote its output", n, 0);
        if (st == FMHIP_OK) st = st2;
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a selection left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(vm); rel(vx); rel(fits);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: select done\n", cycle);
        std::fflush(stdout);
    });
    if (plain) {                                                                // a device list of ONE shard is that shard's call
        const int device = 0;
        OK(fmhip_init_devices(&device, 1));
        scenario(false, false);
        OK(fmhip_shutdown());
        std::printf("a device list of one shard: checked\n");
    }
    return 0;
}
