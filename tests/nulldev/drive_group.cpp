// drive_group.cpp — drives fmhip_group_sums through the C-ABI on the TEST-ONLY null device under the sanitizers.  The vectors hold real
// data and the stand-ins of null_group.cpp scan chunk by chunk with a carry, the kernels' way, so results are CHECKED against the
// definition (fmhip_group_sums_host) bit for bit: every index family, m = 1, 2, 255, 256, 257, 65 537, n and 2^24 (one, two, three and four radix
// passes), 0, 1 and 4 value vectors, every mask, counts and the ungrouped count on and off, at n = 1, 65, one tile + 1, the smallest n with
// two and with three chunks and 40 007 (scratch and stage grow between the calls), and 65 and 1 again behind the large one; hostile
// indices; values with NaN, ±inf and -0.0; pending operands; every argument error that is found on the host.  Twice, with a shutdown and
// a re-initialisation in between; then once more behind a device list of ONE shard.  FMNULL_DEVICES=N: behind N shards every call is
// FMHIP_ERR_UNSUPPORTED and leaves nothing behind; FMNULL_THREAD_ENGINES=1: the calls come from a thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one call in which a pool allocation fails — among the sort's four
// temporaries or the outputs.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"
#include "../../finmath-lib-cuda-extensions_amd/csrc/group_host.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(const F& a, const float* b, int64_t count) { return count == 0 || std::memcmp(a.data(), b, (size_t)count * 4) == 0; }

static const int FAMILIES = 7;
static F index_of(int64_t n, int64_t m, int family, uint32_t seed) {
    F x((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float odd[8] = { nan, inf, -inf, -1.f, 0.5f, (float)m, 1073741824.f, -0.f };
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        const int64_t u = (int64_t)(s >> 8);
        float k;
        switch (family) {
        case 0: k = 0.f; break;                                                   // one group: the prefix total
        case 1: k = (float)((p * 7919 + 3) % n % m); break;                        // a permutation where m == n
        case 2: k = (float)(p * m / n); break;                                     // sorted runs
        case 3: k = (float)(u % m); break;                                         // uniform
        case 4: k = u % 100 ? (float)(m / 2) : (float)(u / 100 % m); break;        // one group holds 99 %
        case 5: k = (float)(u % 3 * (m / 3)); break;                               // many empty groups
        default: k = u % 4 ? (float)(u % m) : odd[(u >> 4) % 8];                   // hostile indices among good ones
        }
        x[(size_t)p] = k;
    }
    return x;
}
static F data(int64_t n, uint32_t seed) {          // values with NaN, ±inf and -0.0 among them
    F a((size_t)n);
    uint32_t s = seed * 747796405u + 2891336453u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = ((float)(s >> 8) * (1.0f / 16777216.0f) - 0.45f) * 1000.f;
        if (p % 1009 == 7) x = std::numeric_limits<float>::quiet_NaN();
        if (p % 1013 == 9) x = std::numeric_limits<float>::infinity();
        if (p % 1019 == 11) x = -std::numeric_limits<float>::infinity();
        if (p % 7 == 3) x = -0.f;
        a[(size_t)p] = x;
    }
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static int64_t size_of(V h) { int64_t n = -1; OK(fmhip_vec_size(h, &n)); return n; }
static fmhip_pool_stats_t pool() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st; }
static int64_t live() { return pool().n_live_vectors; }
static int outputs(uint32_t mask) { return (int)((mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u)); }

// the call with k of the vectors against the definition
static void check(V vi, const F& index, int64_t m, const std::vector<V>& vx, const std::vector<F>& x, int k, uint32_t mask, bool want_counts, bool want_ungrouped) {
    const int64_t n = (int64_t)index.size();
    const int per = outputs(mask), n_out = k * per;
    std::vector<F> want((size_t)n_out, F((size_t)m));
    F want_counts_host((size_t)m);
    const float* in[4]; float* columns[12];
    for (int i = 0; i < k; ++i) in[i] = x[(size_t)i].data();
    for (int i = 0; i < n_out; ++i) columns[i] = want[(size_t)i].data();
    int64_t ungrouped_host = -1, ungrouped = -1;
    OK(fmhip_group_sums_host(index.data(), n, m, in, k, mask, want_counts_host.data(), columns, &ungrouped_host));
    V out[12] = { -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1 }, vc = -1;
    OK(fmhip_group_sums(vi, m, vx.data(), k, mask, want_counts ? &vc : nullptr, out, want_ungrouped ? &ungrouped : nullptr));
    if (want_ungrouped && ungrouped != ungrouped_host) die("the ungrouped count", n, ungrouped);
    if (want_counts) {
        if (size_of(vc) != m || !same(download(vc, m), want_counts_host.data(), m)) die("the counts", n, m);
        rel(vc);
    }
    for (int i = 0; i < n_out; ++i) {
        if (size_of(out[i]) != m) die("the size of an output", n, size_of(out[i]));
        const F got = download(out[i], m);
        if (!same(got, want[(size_t)i].data(), m)) {
            int64_t at = 0; while (std::memcmp(&got[(size_t)at], &want[(size_t)i][(size_t)at], 4) == 0) ++at;
            std::fprintf(stderr, "output %d of mask %u, m = %lld, group %lld: %a, expected %a\n", i, mask, (long long)m, (long long)at, got[(size_t)at], want[(size_t)i][(size_t)at]);
            die("an output", n, i);
        }
        rel(out[i]);
    }
}

static void check_all(const std::vector<V>& vx, const std::vector<F>& x, int64_t n) {
    const int64_t ms[7] = { 1, 2, 255, 256, 257, 65537, n };
    for (int64_t m : ms) {
        if (m == 65537 && n != 65 && n != 4097) continue;                         // (three passes at a small n, below and above one chunk; at the large n: m = n)
        if (n > 5000 && m != 2 && m != 257 && m != n) continue;                 // (one, two and three passes at the large n)
        for (int family = 0; family < FAMILIES; ++family) {
            if (n > 5000 && (family == 1 || family == 5) && m != n) continue;
            const F index = index_of(n, m, family, (uint32_t)(n + 31 * m + family));
            V vi = upload(index);
            check(vi, index, m, vx, x, 1, 7u, true, true);
            check(vi, index, m, vx, x, 0, 0u, true, false);
            check(vi, index, m, vx, x, 0, 0u, false, true);
            if (n < 5000 || family == 6) {
                for (uint32_t mask = 1; mask <= 6; ++mask) check(vi, index, m, vx, x, 1, mask, false, (mask & 1u) != 0u);
                check(vi, index, m, vx, x, 4, 5u, true, true);
                check(vi, index, m, vx, x, 4, 2u, false, false);
            }
            if (!same(download(vi, n), index.data(), n)) die("the index changed", n, family);
            rel(vi);
        }
    }
    if (n == 65) {                                                                // m = 2^24: the key of an ungrouped element needs a FOURTH radix pass
        const int64_t m = int64_t(1) << 24;
        const F index = index_of(n, m, 6, 99u);                                   // NaN, ±inf, negative, a fraction, m and 2^30 among good indices
        V vi = upload(index);
        check(vi, index, m, vx, x, 0, 0u, true, true);                            // (the counts and the ungrouped count: one vector of 2^24 elements)
        rel(vi);
    }
    if (!same(download(vx[0], n), x[0].data(), n)) die("a value vector changed", n, 0);
}

static void refusals(V vx, int64_t n) {
    V vi = upload(index_of(n, 5, 3, 5)), longer = upload(F((size_t)n + 1, 1.f));
    const fmhip_pool_stats_t before = pool();
    V out[12] = { 0 }, vc = 0; int64_t u = -7;
    V five[5] = { vx, vx, vx, vx, vx }, with_zero[2] = { vx, 0 };
    const int bad = FMHIP_ERR_INVALID_ARGUMENT;
    EXPECT(fmhip_group_sums(vi, 0, &vx, 1, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, (int64_t(1) << 24) + 1, &vx, 1, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, five, 5, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, &vx, -1, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, &vx, 1, 0u, &vc, out, &u), bad);                          // a mask of 0 with a value vector
    EXPECT(fmhip_group_sums(vi, 5, &vx, 1, 8u, &vc, out, &u), bad);                          // unknown bits
    EXPECT(fmhip_group_sums(vi, 5, nullptr, 0, 0u, nullptr, nullptr, nullptr), bad);         // nothing asked for
    EXPECT(fmhip_group_sums(0, 5, &vx, 1, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, nullptr, 1, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, &vx, 1, 1u, &vc, nullptr, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, with_zero, 2, 1u, &vc, out, &u), bad);
    EXPECT(fmhip_group_sums(vi, 5, &longer, 1, 1u, &vc, out, &u), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_group_sums(vi + 12345, 5, &vx, 1, 1u, &vc, out, &u), FMHIP_ERR_INVALID_HANDLE);
    const fmhip_pool_stats_t after = pool();
    if (out[0] != 0 || vc != 0 || u != -7 || after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", n, after.n_live_vectors - before.n_live_vectors);
    rel(vi); rel(longer);
}

static void unsupported(V vx, int64_t n) {
    V vi = upload(index_of(n, 5, 3, 5));
    const int64_t before = live();
    V out = 0, vc = 0; int64_t u = -7;
    EXPECT(fmhip_group_sums(vi, 5, &vx, 1, 1u, &vc, &out, &u), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_group_sums(vi, 5, nullptr, 0, 0u, nullptr, nullptr, &u), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_group_sums(vi, 5, &vx, 5, 1u, &vc, &out, &u), FMHIP_ERR_INVALID_ARGUMENT);  // the checks still come first
    EXPECT(fmhip_group_sums(vi, 0, &vx, 1, 1u, &vc, &out, &u), FMHIP_ERR_INVALID_ARGUMENT);
    if (out != 0 || vc != 0 || u != -7 || live() != before) die("a device list of several shards left something behind", n, live() - before);
    rel(vi);
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t TWO = fm::prefix_chunk_elems(1) + 1, THREE = 2 * fm::prefix_chunk_elems(1) + 1;
    if (fm::prefix_blocks(TWO) != 2 || fm::prefix_blocks(TWO - 1) != 1 || fm::prefix_blocks(THREE) != 3) die("the smallest n with two and three chunks", TWO, THREE);
    const int64_t sizes[8] = { 1, 65, fm::FM_PREFIX_TILE + 1, TWO, THREE, 40007, 65, 1 };
    for (int64_t n : sizes) {
        std::vector<F> x; std::vector<V> vx;
        for (int i = 0; i < 4; ++i) { x.push_back(data(n, (uint32_t)(n + 1 + i))); vx.push_back(upload(x.back())); }
        if (sharded) unsupported(vx[0], n);
        else {
            const int64_t before = live();
            if (thread_engines) {
                std::thread asker([&] { check_all(vx, x, n); });                         // a thread that owns none of them
                asker.join();
                if (n < 5000) check_all(vx, x, n);                                     // and the owner
            }
            else check_all(vx, x, n);
            if (n == 65 || n == THREE) refusals(vx[0], n);
            if (live() != before) die("the calls left vectors behind", n, live() - before);
        }
        for (V h : vx) rel(h);
    }
    if (sharded) return;
    // pending operands: the results against what the vectors hold once they exist
    const int64_t n = THREE, m = 300;
    V stored = upload(index_of(n, m, 6, 7)), state = upload(data(n, 8));
    V pending_i = 0, pending_x = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0, &pending_i));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, state, 1.0, &pending_x));
    V outs[3] = { 0, 0, 0 }, vc = 0; int64_t ungrouped = -1;
    OK(fmhip_group_sums(pending_i, m, &pending_x, 1, 7u, &vc, outs, &ungrouped));
    {
        const F index = download(pending_i, n), x = download(pending_x, n);
        std::vector<F> want(3, F((size_t)m)); F counts((size_t)m);
        const float* in[1] = { x.data() }; float* columns[3] = { want[0].data(), want[1].data(), want[2].data() }; int64_t ungrouped_host = -1;
        OK(fmhip_group_sums_host(index.data(), n, m, in, 1, 7u, counts.data(), columns, &ungrouped_host));
        if (ungrouped != ungrouped_host || !same(download(vc, m), counts.data(), m)) die("the counts of pending vectors", n, 0);
        for (int j = 0; j < 3; ++j) if (!same(download(outs[j], m), want[(size_t)j].data(), m)) die("the group sums of pending vectors", n, j);
    }
    for (V h : outs) rel(h);
    rel(vc); rel(stored); rel(state); rel(pending_i); rel(pending_x);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller.  A call with one value vector, two outputs and the counts takes SEVEN pool allocations:
// the sort's four temporaries, the counts and the two outputs.  Without the variable this is the counting run.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 9001, m = 300;
    V vi = upload(index_of(n, m, 6, 5)), vx = upload(data(n, 6));
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V outs[2] = { 0, 0 }, vc = 0; int64_t u = -7;
        const int st = fmhip_group_sums(vi, m, &vx, 1, 3u, &vc, outs, &u);
        if (st == FMHIP_OK) { rel(outs[0]); rel(outs[1]); rel(vc); }
        else if (outs[0] != 0 || outs[1] != 0 || vc != 0 || u != -7) die("a failed call wrote its outputs", n, 0);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a group call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(vi); rel(vx);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: group done\n", cycle);
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
