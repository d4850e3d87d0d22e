// drive_cross_order.cpp — drives fmhip_cross_order_statistics and fmhip_cross_select through the C-ABI on the TEST-ONLY null device under the
// sanitizers.  The vectors hold real data — NaNs with payloads, both infinities, signed zeros, ties across slots, the same handle in two
// slots — and the stand-ins of null_cross_order.cpp sort with the kernels' network and range-check the index as the kernel does, so
// results are CHECKED against the definition (the _host calls): every padded network size with its neighbours (K = 1, 2, 3, 4, 5, 8, 9, 16,
// 17, 31, 32), all ranks with a duplicate, values, indices and both, the selection behind an index output and behind indices that name
// no slot.  Pending operands, operands whose inputs another thread releases during the call, every argument error that is found on the
// host.  Twice, with a shutdown and a re-initialisation in between; then once more behind a device list of ONE shard.
// FMNULL_DEVICES=N: behind N shards the calls run per shard and give the same results; FMNULL_THREAD_ENGINES=1: the calls come from a
// thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_cross_order_statistics in which the allocation of an output fails.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// signed values over sixteen decades with zeros of both signs and ties ACROSS slots (a value that depends on the path alone); special: NaNs
// of both signs with payloads and both infinities
static F data(int64_t n, uint32_t seed, bool special) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (s & 16u) x = -x;
        if (p % 5 == 2) x = (s & 32u) ? 0.f : -0.f;
        if (p % 7 == 3) x = 1.5f + (float)(p % 3);
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

static void expect_columns(const V* outs, const std::vector<F>& want, int64_t n, const char* what) {
    for (size_t o = 0; o < want.size(); ++o) {
        if (size_of(outs[o]) != n) die("the size of an output", n, (int64_t)o);
        const F got = download(outs[o], n);
        for (int64_t p = 0; p < n; ++p) if (!same(got[(size_t)p], want[o][(size_t)p])) die(what, n, (int64_t)o * 1000000 + p);
    }
}
static std::vector<F> host_statistics(const std::vector<F>& as, int64_t n, const std::vector<int>& ranks, int outputs) {
    std::vector<const float*> in; for (const F& a : as) in.push_back(a.data());
    std::vector<F> want((size_t)((int)ranks.size() * ((outputs & 1) + (outputs >> 1))), F((size_t)n, -1.f));
    std::vector<float*> out; for (F& w : want) out.push_back(w.data());
    OK(fmhip_cross_order_statistics_host(in.data(), (int)as.size(), n, ranks.data(), (int)ranks.size(), outputs, out.data()));
    return want;
}

// vs[i] holds as[i]; the same handle may stand in several slots
static void check_calls(const std::vector<V>& vs, const std::vector<F>& as, int64_t n) {
    const int K = (int)vs.size();
    std::vector<int> ranks; for (int r = 0; r < K; ++r) ranks.push_back(r);
    if (K < 32) ranks.push_back(K / 2);                                                              // a duplicate
    for (int outputs = 1; outputs <= 3; ++outputs) {
        const std::vector<F> want = host_statistics(as, n, ranks, outputs);
        std::vector<V> outs(want.size(), 0);
        OK(fmhip_cross_order_statistics(vs.data(), K, ranks.data(), (int)ranks.size(), outputs, outs.data()));
        expect_columns(outs.data(), want, n, "cross order statistics");
        if (outputs == 2) {                                                                          // the selection behind the median's index
            std::vector<const float*> in; for (const F& a : as) in.push_back(a.data());
            F want_pick((size_t)n, -1.f);
            OK(fmhip_cross_select_host(want[(size_t)(K / 2)].data(), in.data(), K, n, want_pick.data()));
            V pick = 0;
            OK(fmhip_cross_select(outs[(size_t)(K / 2)], vs.data(), K, &pick));
            expect_columns(&pick, { want_pick }, n, "cross select");
            rel(pick);
        }
        for (V h : outs) rel(h);
    }
    // indices that name no slot
    F index((size_t)n);
    const float odd[8] = { -1.f, (float)K, 0.5f, std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), -0.f, (float)(K - 1) };
    for (int64_t p = 0; p < n; ++p) index[(size_t)p] = odd[p % 8];
    std::vector<const float*> in; for (const F& a : as) in.push_back(a.data());
    F want_pick((size_t)n, -1.f);
    OK(fmhip_cross_select_host(index.data(), in.data(), K, n, want_pick.data()));
    V vi = upload(index), pick = 0;
    OK(fmhip_cross_select(vi, vs.data(), K, &pick));
    expect_columns(&pick, { want_pick }, n, "cross select of odd indices");
    rel(pick); rel(vi);
}

static void refusals(V v, V other_size, int64_t n) {
    const int64_t before = live();
    V outs[64] = { 0 }; V out = 0;
    std::vector<V> many(33, v);
    const V two[2] = { v, v }, mixed[2] = { v, other_size }, with_zero[2] = { v, 0 }, unknown[1] = { v + 12345 };
    int r[33] = { 0 }; const int one[1] = { 1 }, two_[1] = { 2 }, minus[1] = { -1 };
    EXPECT(fmhip_cross_order_statistics(two, 0, r, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(many.data(), 33, r, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, 0, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, 33, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, -1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, two_, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);      // rank K
    EXPECT(fmhip_cross_order_statistics(two, 1, one, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, minus, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, 1, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, 1, 4, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(nullptr, 2, r, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, nullptr, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(two, 2, r, 1, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(with_zero, 2, r, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_order_statistics(mixed, 2, r, 1, 1, outs), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_order_statistics(unknown, 1, r, 1, 1, outs), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_cross_select(0, two, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(v, two, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(v, many.data(), 33, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(v, nullptr, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(v, two, 2, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(v, with_zero, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_select(other_size, two, 2, &out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_select(v, mixed, 2, &out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_select(v + 12345, two, 2, &out), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_cross_select(v, unknown, 1, &out), FMHIP_ERR_INVALID_HANDLE);
    for (V h : outs) if (h != 0) die("a refused call wrote an output", n, 0);
    if (out != 0 || live() != before) die("a refused call left something behind", n, live() - before);
}

static void shapes_checked() {
    const int Ks[] = { 1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32 };
    const int64_t ns[] = { 1, 65, 2049 };
    for (int K : Ks) for (int64_t n : ns) {
        if (K > 9 && n > 65) continue;
        std::vector<F> as; std::vector<V> vs;
        for (int i = 0; i < K; ++i) {
            if (i == K - 1 && K >= 2) { as.push_back(as[0]); vs.push_back(vs[0]); continue; }         // the same handle in two slots
            as.push_back(data(n, (uint32_t)(n + 31 * i + K), i % 3 != 2)); vs.push_back(upload(as.back()));
        }
        const int64_t before = live();
        check_calls(vs, as, n);
        if (live() != before) die("the calls left vectors behind", n, live() - before);
        for (int i = 0; i < K; ++i) if (!(i == K - 1 && K >= 2)) rel(vs[(size_t)i]);
    }
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 4097;
    const F a = data(n, 11, true), b = data(130, 12, false);
    V va = upload(a), vb = upload(b);
    if (thread_engines) {
        std::thread asker([&] { shapes_checked(); });                                                // a thread that owns none of the vectors it makes here … (its engine is its own)
        asker.join();
    }
    shapes_checked();
    refusals(va, vb, n);
    // pending operands: the results against what the vectors hold once they exist
    V p1 = 0, p2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, vb, 2.0, &p1));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 1.0, &p2));
    {
        const std::vector<V> pend = { p1, vb, p2 };
        V probe[2] = { 0, 0 };
        const int r[1] = { 2 };
        OK(fmhip_cross_order_statistics(pend.data(), 3, r, 1, 3, probe));                            // first on the pending vectors …
        std::vector<F> held;
        for (V h : pend) held.push_back(download(h, 130));
        expect_columns(probe, host_statistics(held, 130, { 2 }, 3), 130, "cross order statistics of pending vectors");
        rel(probe[0]); rel(probe[1]);
        if (thread_engines) { std::thread asker([&] { check_calls(pend, held, 130); }); asker.join(); }      // … from a thread that owns none of them
        check_calls(pend, held, 130);                                                                // … then on the stored ones
    }
    rel(p1); rel(p2);
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
    V outs[2] = { 0 }, pick = 0;
    const int r[1] = { 3 };
    OK(fmhip_cross_order_statistics(derived.data(), 4, r, 1, 3, outs));
    OK(fmhip_cross_select(outs[1], derived.data() + 2, 4, &pick));
    releaser.join();
    for (V h : outs) rel(h);
    rel(pick);
    for (V d : derived) rel(d);
    rel(va); rel(vb);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the outputs of one fmhip_cross_order_statistics are its pool allocations (six here).  Without
// it this is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5000;
    const std::vector<F> as = { data(n, 5, true), data(n, 6, false), data(n, 7, true) };
    const V vs[3] = { upload(as[0]), upload(as[1]), upload(as[2]) };
    const std::vector<int> ranks = { 0, 2, 2 };
    const std::vector<F> want = host_statistics(as, n, ranks, 3);
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V outs[6] = { 0, 0, 0, 0, 0, 0 };
        const int st = fmhip_cross_order_statistics(vs, 3, ranks.data(), 3, 3, outs);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) { expect_columns(outs, want, n, "cross order statistics"); for (V h : outs) rel(h); }
        else for (V h : outs) if (h != 0) die("a failed call wrote its outputs", n, 0);
        V pick = 0;
        const int rs = fmhip_cross_select(vs[0], vs, 3, &pick);
        if (rs == FMHIP_OK) rel(pick); else if (pick != 0) die("a failed cross select wrote its output", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a cross order pass left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    for (V h : vs) rel(h);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: cross order done\n", cycle);
        std::fflush(stdout);
    });
    if (plain) {                                                                // a device list of ONE shard is that shard's call
        const int device = 0;
        OK(fmhip_init_devices(&device, 1));
        scenario(false);
        OK(fmhip_shutdown());
        std::printf("a device list of one shard: checked\n");
    }
    return 0;
}
