// drive_block_order.cpp — drives fmhip_block_order_statistics and fmhip_block_sort through the C-ABI on the TEST-ONLY null device under the
// sanitizers.  The vectors hold real data — NaNs with payloads, both infinities, signed zeros, ties — and the stand-in of
// null_block_order.cpp sorts the padded keys and sums a range as a wave does, so results are CHECKED against the definition (the _host
// calls): ranks with a duplicate, ranges of one term, of the whole block and across the 2048-term segment, one and four vectors per
// call, blocks of both regimes and around their boundaries (1, 3, 64, 65, 128, 129, 2049, 4096), a small shape again behind the large
// one.  Pending operands, operands whose inputs another thread releases during the call, every argument error that is found on the host.
// Twice, with a shutdown and a re-initialisation in between; then once more behind a device list of ONE shard.
// FMNULL_DEVICES=N: behind N shards every call is FMHIP_ERR_UNSUPPORTED and leaves nothing behind; FMNULL_THREAD_ENGINES=1: the calls come
// from a thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_block_order_statistics in which the allocation of an output fails.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
typedef std::vector<int64_t> I;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// signed values over sixteen decades with zeros of both signs and ties; special: NaNs of both signs with payloads and both infinities
static F data(int64_t n, uint32_t seed, bool special) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (p % 5 == 2) x = 0.f;
        if (p % 7 == 3) x = 1.5f;
        if (s & 16u) x = -x;
        a[(size_t)p] = x;
    }
    if (special) {
        const uint32_t payload = 0x7fc12345u, negative = 0xffa00001u;
        std::memcpy(&a[0], &payload, 4);
        if (n > 4) std::memcpy(&a[(size_t)n - 2], &negative, 4);
        if (n > 2) a[(size_t)n / 2] = std::numeric_limits<float>::infinity();
        if (n > 8) a[(size_t)n / 2 + 1] = -std::numeric_limits<float>::infinity();
    }
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static int64_t size_of(V h) { int64_t n = -1; OK(fmhip_vec_size(h, &n)); return n; }
static int64_t live() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st.n_live_vectors; }

struct Select { I ranks, from, to; };
static Select selectors(int64_t block) {
    Select s;
    s.ranks = { 0, block - 1, block / 2, 0 };
    s.from = { 0, 0, block / 2 }; s.to = { 0, block - 1, block - 1 };
    if (block > 2050) { s.from.push_back(1); s.to.push_back(2049); }                      // one more term than a segment, not from the start
    return s;
}

static void check_statistics(const std::vector<V>& vs, const std::vector<F>& as, int64_t block) {
    const int64_t n = (int64_t)as[0].size(), m = n / block;
    const Select s = selectors(block);
    const int nr = (int)s.ranks.size(), ng = (int)s.from.size(), k = nr + ng;
    std::vector<V> outs(vs.size() * (size_t)k, 0);
    OK(fmhip_block_order_statistics(vs.data(), (int)vs.size(), block, s.ranks.data(), nr, s.from.data(), s.to.data(), ng, outs.data()));
    for (size_t i = 0; i < vs.size(); ++i) {
        F want((size_t)(k * m), -1.f);
        OK(fmhip_block_order_statistics_host(as[i].data(), n, block, s.ranks.data(), nr, s.from.data(), s.to.data(), ng, want.data()));
        for (int j = 0; j < k; ++j) {
            const V h = outs[i * (size_t)k + (size_t)j];
            if (size_of(h) != m) die("the size of an output", n, block);
            const F got = download(h, m);
            for (int64_t q = 0; q < m; ++q) if (!same(got[(size_t)q], want[(size_t)(j * m + q)])) die("block order statistics", block, j * 1000000 + q);
            rel(h);
        }
        V sorted = 0;
        OK(fmhip_block_sort(vs[i], block, &sorted));
        if (size_of(sorted) != n) die("the size of a block sort", n, block);
        F want_sorted((size_t)n, -1.f);
        OK(fmhip_block_sort_host(as[i].data(), n, block, want_sorted.data()));
        const F got = download(sorted, n);
        for (int64_t p = 0; p < n; ++p) if (!same(got[(size_t)p], want_sorted[(size_t)p])) die("block sort", block, p);
        rel(sorted);
    }
    // ranks alone, ranges alone
    OK(fmhip_block_order_statistics(vs.data(), 1, block, s.ranks.data(), 1, nullptr, nullptr, 0, outs.data())); rel(outs[0]);
    OK(fmhip_block_order_statistics(vs.data(), 1, block, nullptr, 0, s.from.data(), s.to.data(), 1, outs.data())); rel(outs[0]);
}

static void refusals(V v, V other_size, int64_t n) {
    const int64_t before = live();
    V outs[48] = { 0 }; V out = 0;
    const V two[2] = { v, v }, mixed[2] = { v, other_size }, with_zero[2] = { v, 0 }, five[5] = { v, v, v, v, v }, unknown[1] = { v + 12345 };
    const int64_t r[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, lo[5] = { 0, 0, 0, 0, 0 }, hi[5] = { 0, 0, 0, 0, 0 }, one[1] = { 1 }, minus[1] = { -1 }, two_[1] = { 2 }, big[1] = { n };
    EXPECT(fmhip_block_order_statistics(two, 0, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(five, 5, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 9, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, -1, lo, hi, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, hi, 5, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, hi, -1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, one, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);        // rank 1 of a block of 1
    EXPECT(fmhip_block_order_statistics(two, 2, 1, minus, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, one, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);         // a range outside the block
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, minus, hi, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, n, r, 0, two_, one, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);       // from > to
    EXPECT(fmhip_block_order_statistics(two, 2, 0, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, -3, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, n > 2 ? n - 1 : 2, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(nullptr, 1, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 1, lo, hi, 0, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, nullptr, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, nullptr, hi, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, nullptr, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(with_zero, 2, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_order_statistics(mixed, 2, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_block_order_statistics(unknown, 1, 1, r, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_block_order_statistics(two, 2, 4097, r, 1, lo, hi, 0, outs), FMHIP_ERR_UNSUPPORTED);            // no kernel for such a block, whatever n
    if (std::string(fmhip_last_error()).find("fmhip_select_ranks_batch") == std::string::npos || std::string(fmhip_last_error()).find("fmhip_sort_by_key") == std::string::npos) die("the message of a long block", n, 0);
    EXPECT(fmhip_block_order_statistics(two, 2, 4097, big, 1, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);     // … but a rank outside it is said first
    EXPECT(fmhip_block_sort(v, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_sort(v, -1, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_sort(v, n > 2 ? n - 1 : 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_sort(v, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_sort(0, 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_sort(v + 12345, 1, &out), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_block_sort(v, 5000, &out), FMHIP_ERR_UNSUPPORTED);
    for (V h : outs) if (h != 0) die("a refused call wrote an output", n, 0);
    if (out != 0 || live() != before) die("a refused call left something behind", n, live() - before);
}

static void unsupported(V v, int64_t n) {
    const int64_t before = live();
    V outs[12] = { 0 }; V out = 0;
    const V two[2] = { v, v };
    const int64_t r[2] = { 0, 0 }, lo[1] = { 0 }, hi[1] = { 0 };
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 2, lo, hi, 1, outs), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_block_order_statistics(two, 1, n, r, 1, lo, hi, 0, outs), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_block_sort(v, 1, &out), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_block_order_statistics(two, 2, 1, r, 0, lo, hi, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);      // what needs no look at a vector is still said first
    EXPECT(fmhip_block_sort(v, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
    for (V h : outs) if (h != 0) die("a device list of several shards wrote an output", n, 0);
    if (out != 0 || live() != before) die("a device list of several shards left something behind", n, live() - before);
}

struct Shape { int64_t block, m; };

static void shapes_checked(bool four) {
    // small (1, 3, 64), medium (65 … 4096: P = 128, 256, 4096 with a range across the segment boundary), then small again
    const Shape shapes[] = { { 1, 67 }, { 3, 23 }, { 64, 5 }, { 65, 3 }, { 128, 2 }, { 129, 3 }, { 2049, 2 }, { 4096, 2 }, { 7, 9 } };
    for (const Shape& sh : shapes) {
        const int64_t n = sh.block * sh.m;
        std::vector<F> as; std::vector<V> vs;
        for (int i = 0; i < (four ? 4 : 1); ++i) { as.push_back(data(n, (uint32_t)(n + i), i != 2)); vs.push_back(upload(as.back())); }
        const int64_t before = live();
        check_statistics(vs, as, sh.block);
        if (live() != before) die("the calls left vectors behind", n, live() - before);
        for (V h : vs) rel(h);
    }
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 4097;
    const F a = data(n, 11, true), b = data(130, 12, false);
    V va = upload(a), vb = upload(b);
    if (sharded) { unsupported(va, n); unsupported(vb, 130); rel(va); rel(vb); return; }
    if (thread_engines) {
        std::thread asker([&] { shapes_checked(true); });                                  // a thread that owns none of the vectors it is not given
        asker.join();
        shapes_checked(false);
    } else { shapes_checked(true); shapes_checked(false); }
    refusals(va, vb, n);
    // pending operands: the results against what the vectors hold once they exist
    V p1 = 0, p2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, vb, 2.0, &p1));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 1.0, &p2));
    {
        const std::vector<V> pend = { p1, p2 };
        std::vector<F> held;
        V probe[2] = { 0, 0 };
        const int64_t r[1] = { 12 };
        OK(fmhip_block_order_statistics(pend.data(), 2, 13, r, 1, nullptr, nullptr, 0, probe));      // first on the pending vectors …
        for (V h : pend) held.push_back(download(h, 130));
        for (int i = 0; i < 2; ++i) {
            F want(10);
            OK(fmhip_block_order_statistics_host(held[(size_t)i].data(), 130, 13, r, 1, nullptr, nullptr, 0, want.data()));
            const F got = download(probe[i], 10);
            for (int q = 0; q < 10; ++q) if (!same(got[(size_t)q], want[(size_t)q])) die("block order statistics of a pending vector", 130, q);
            rel(probe[i]);
        }
        check_statistics(pend, held, 13);                                                            // … then on the stored ones
    }
    V p3 = 0, sorted = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, vb, 3.0, &p3));
    OK(fmhip_block_sort(p3, 26, &sorted));
    { const F held = download(p3, 130), got = download(sorted, 130); F want(130); OK(fmhip_block_sort_host(held.data(), 130, 26, want.data())); for (int o = 0; o < 130; ++o) if (!same(got[(size_t)o], want[(size_t)o])) die("block sort of a pending vector", 130, o); }
    rel(sorted); rel(p1); rel(p2); rel(p3);
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    V outs[4] = { 0 };
    const int64_t r[1] = { 9 };
    OK(fmhip_block_order_statistics(derived.data(), 4, 10, r, 1, nullptr, nullptr, 0, outs));
    OK(fmhip_block_sort(derived[5], 65, &sorted));
    releaser.join();
    for (V h : outs) rel(h);
    rel(sorted);
    for (V d : derived) rel(d);
    rel(va); rel(vb);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the outputs of one fmhip_block_order_statistics are its pool allocations (six here).  Without
// it this is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5000, block = 50, m = n / block;
    const F a = data(n, 5, true), b = data(n, 6, false);
    const V vs[2] = { upload(a), upload(b) };
    const int64_t r[2] = { 0, 49 }, lo[1] = { 0 }, hi[1] = { 4 };
    F want_a((size_t)(3 * m)), want_b((size_t)(3 * m));
    OK(fmhip_block_order_statistics_host(a.data(), n, block, r, 2, lo, hi, 1, want_a.data()));
    OK(fmhip_block_order_statistics_host(b.data(), n, block, r, 2, lo, hi, 1, want_b.data()));
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V outs[6] = { 0, 0, 0, 0, 0, 0 };
        const int st = fmhip_block_order_statistics(vs, 2, block, r, 2, lo, hi, 1, outs);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            for (int k = 0; k < 6; ++k) {
                const F got = download(outs[k], m); const F& want = k < 3 ? want_a : want_b;
                for (int64_t q = 0; q < m; ++q) if (!same(got[(size_t)q], want[(size_t)((k % 3) * m + q)])) die("block order statistics", n, q);
                rel(outs[k]);
            }
        } else for (V h : outs) if (h != 0) die("a failed call wrote its outputs", n, 0);
        V sorted = 0;
        const int rs = fmhip_block_sort(vs[0], block, &sorted);
        if (rs == FMHIP_OK) rel(sorted); else if (sorted != 0) die("a failed block sort wrote its output", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a block order pass left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(vs[0]); rel(vs[1]);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: block order done\n", cycle);
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
