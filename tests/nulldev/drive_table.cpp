// drive_table.cpp — drives fmhip_table_apply through the C-ABI on the TEST-ONLY null device under the sanitizers: vectors of real data at sizes
// around the kernel's tile and group, uniform / geometric / two-cluster knots with 1 … 1024 of them, all four interpolations and the
// derivative, 1 … 4 tables per call up to the knots x tables limit, every result compared bit for bit with fmhip_table_apply_host (the
// stand-in launcher of null_table.cpp searches THE KERNEL'S WAY, by the index the engine built); a pending (fused, unflushed) x, a given-up x,
// a second thread releasing the inputs of pending operands during the call, every argument refusal with nothing launched and nothing left
// behind.  Twice, with a shutdown and a re-initialisation in between; then behind a device list of ONE shard.  FMNULL_DEVICES=N: behind a
// device list of N shards (every shard its block); FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vector asked about by a thread
// that does not own it.  `failure`: FMHIP_TEST_FAIL_ALLOC_AT on each of the output allocations.
// The null device computes nothing element-wise, so a pending operand is compared with what its buffer holds once it exists.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
typedef std::vector<double> D;
static V upload(const F& v) { V h = 0; OK(fmhip_vec_create_from_float(v.data(), (int64_t)v.size(), &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static fmhip_pool_stats_t stats() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st; }

// kind 0: uniform, 1: geometric over twelve decades, 2: two clusters far apart
static D knots_of(int m, int kind) {
    D k((size_t)m);
    for (int i = 0; i < m; ++i)
        k[(size_t)i] = kind == 0 ? -3.0 + 0.1 * i : kind == 1 ? 1e-6 * std::pow(1e12, m > 1 ? (double)i / (m - 1) : 0.0) : (i < m / 2 ? -100.0 + 1e-3 * i : 100.0 + 1e-3 * i);
    return k;
}
static F data(int64_t n, const D& k, unsigned seed) {
    F a((size_t)n);
    const double lo = k.front(), hi = k.back(), span = hi > lo ? hi - lo : 1.0;
    uint64_t s = 0x9e3779b97f4a7c15ull * (seed + 1);
    for (int64_t p = 0; p < n; ++p) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(s >> 11) * 0x1.0p-53;
        a[(size_t)p] = p % 7 == 3 ? (float)k[(size_t)((s >> 20) % k.size())] : (float)(lo - 0.1 * span + 1.2 * span * u);      // on a knot, or across the range and beyond
    }
    const float edge[] = { 0.0f, -0.0f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(),
                           std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max() };
    for (size_t e = 0; e < sizeof edge / sizeof *edge && (int64_t)e < n; ++e) a[(size_t)((e * 977) % (size_t)n)] = edge[e];
    return a;
}
static D table(const D& k, int interpolation, int extrapolation, int derivative, int which) {
    D v(k.size()), c((k.size() + 1) * 4);
    for (size_t i = 0; i < k.size(); ++i) v[i] = std::sin(0.37 * (double)i + which) + 0.01 * (double)i * which;
    OK(fmhip_table_build(k.data(), v.data(), (int)k.size(), interpolation, extrapolation, derivative, c.data()));
    return c;
}

static void check(V hx, const F& x, const D& k, int T, int variant) {
    const int64_t n = (int64_t)x.size();
    D coef;
    for (int f = 0; f < T; ++f) { const D c = table(k, (variant + f) % 4, (variant + f / 2) % 2, f == 3 ? 1 : 0, f); coef.insert(coef.end(), c.begin(), c.end()); }
    V out[4] = { 0, 0, 0, 0 };
    OK(fmhip_table_apply(hx, k.data(), (int)k.size(), coef.data(), T, out));
    std::vector<F> want((size_t)T, F((size_t)n));
    float* cols[4] = { nullptr, nullptr, nullptr, nullptr };
    for (int f = 0; f < T; ++f) cols[f] = want[(size_t)f].data();
    OK(fmhip_table_apply_host(x.data(), n, k.data(), (int)k.size(), coef.data(), T, cols));
    for (int f = 0; f < T; ++f) {
        int64_t size = -1; OK(fmhip_vec_size(out[f], &size));
        if (size != n) die("the size of a result", n, size);
        const F got = download(out[f], n);
        if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("a tabulated function differs from the definition", n, (int64_t)k.size() * 10 + f);
        rel(out[f]);
    }
}

static void refusals(V x, int64_t n) {
    const fmhip_pool_stats_t before = stats();
    const D k = knots_of(5, 0), c = table(k, 1, 0, 0, 0);
    D c4; for (int f = 0; f < 4; ++f) c4.insert(c4.end(), c.begin(), c.end());
    V out[4] = { 0, 0, 0, 0 };
    const D unsorted = { 0.0, 1.0, 1.0, 2.0, 3.0 }, nan_k = { 0.0, 1.0, std::nan(""), 2.0, 3.0 }, inf_k = { 0.0, 1.0, 2.0, 3.0, std::numeric_limits<double>::infinity() };
    const D k1024 = knots_of(1024, 0), k513 = knots_of(513, 0);
    D big(1025 * 4 * 2, 0.0);
    EXPECT(fmhip_table_apply(0, k.data(), 5, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, nullptr, 5, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k.data(), 5, nullptr, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k.data(), 5, c.data(), 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k.data(), 0, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k1024.data(), 1025, big.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k.data(), 5, c4.data(), 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k.data(), 5, c4.data(), 5, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, k513.data(), 513, big.data(), 2, out), FMHIP_ERR_INVALID_ARGUMENT);      // knots x tables > 1024
    EXPECT(fmhip_table_apply(x, unsorted.data(), 5, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, nan_k.data(), 5, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x, inf_k.data(), 5, c.data(), 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply(x + 1000000, k.data(), 5, c.data(), 1, out), FMHIP_ERR_INVALID_HANDLE);
    // the host-only calls
    D v(5, 1.0), co(6 * 4); const D nan_v = { 1.0, std::nan(""), 1.0, 1.0, 1.0 };
    F hx((size_t)4, 0.5f), ho((size_t)4); float* col[1] = { ho.data() }; float* none[1] = { nullptr };
    EXPECT(fmhip_table_build(nullptr, v.data(), 5, 1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), nullptr, 5, 1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 5, 1, 0, 0, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 0, 1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 5, 4, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 5, -1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 5, 1, 2, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), v.data(), 5, 1, 0, 2, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(k.data(), nan_v.data(), 5, 1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_build(unsorted.data(), v.data(), 5, 1, 0, 0, co.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply_host(nullptr, 4, k.data(), 5, c.data(), 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply_host(hx.data(), 0, k.data(), 5, c.data(), 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply_host(hx.data(), 4, k.data(), 5, c.data(), 1, none), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply_host(hx.data(), 4, k.data(), 5, c.data(), 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_table_apply_host(hx.data(), 4, unsorted.data(), 5, c.data(), 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    if (out[0] != 0) die("a refused call wrote its outputs", n, 0);
    const fmhip_pool_stats_t after = stats();
    if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    if (after.n_alloc_hits + after.n_alloc_misses != before.n_alloc_hits + before.n_alloc_misses) die("a refused call allocated", n, 0);
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099, 100003 };
    int variant = 0;
    for (int64_t n : sizes) {
        for (int kind = 0; kind < 3; ++kind) {
            const int ms[] = { 1, 2, 3, 4, 5, 64, 65, 1023, 1024 };
            for (int m : ms) {
                if (n > 5000 && m != 65 && m != 1024) continue;
                if (n < 1000 && n != 5 && n != 65 && m != 4 && m != 1023) continue;
                const D k = knots_of(m, kind);
                const F x = data(n, k, (unsigned)(n + 31 * m + kind));
                V hx = upload(x);
                const int64_t before = stats().n_live_vectors;
                for (int T = 1; T <= 4; ++T) {
                    if (m * T > 1024) continue;
                    auto run = [&] { check(hx, x, k, T, variant); };
                    if (thread_engines && T % 2 == 0) { std::thread asker(run); asker.join(); }      // a thread that does not own x
                    else run();
                    ++variant;
                }
                if (stats().n_live_vectors != before) die("the calls left vectors behind", n, m);
                rel(hx);
            }
        }
    }
    // T = 4 at the knots x tables limit
    {
        const D k = knots_of(256, 1); const F x = data(3001, k, 5); V hx = upload(x);
        check(hx, x, k, 4, 1);
        refusals(hx, 3001);
        rel(hx);
    }
    // a pending (fused, unflushed) x: the result against what the vector holds once it exists
    const int64_t n = 2051;
    const D k = knots_of(33, 0);
    const F base = data(n, k, 9);
    V stored = upload(base);
    V pending = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &pending));
    {
        const D c = table(k, 2, 1, 0, 0);
        V out[1] = { 0 };
        OK(fmhip_table_apply(pending, k.data(), 33, c.data(), 1, out));
        const F x = download(pending, n);
        F want((size_t)n); float* col[1] = { want.data() };
        OK(fmhip_table_apply_host(x.data(), n, k.data(), 33, c.data(), 1, col));
        const F got = download(out[0], n);
        if (std::memcmp(got.data(), want.data(), (size_t)n * 4) != 0) die("a tabulated function of a pending vector", n, 0);
        rel(out[0]);
    }
    // a given-up x whose values the engine has not kept: the error a read of it is
    if (!sharded && !thread_engines) {
        V gone = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 5.0, &gone));
        OK(fmhip_vec_give_up_values(&gone, 1));
        fmhip_ticket ticket = 0; fmhip_moments mo;
        OK(fmhip_reduce_moments_batch_begin(&gone, 1, nullptr, &ticket));
        OK(fmhip_reduce_moments_batch_end(ticket, &mo, 1));
        F h((size_t)n);
        const int read = fmhip_vec_read_float(gone, h.data(), n);
        const D c = table(k, 1, 0, 0, 0);
        V out[1] = { 0 };
        const int st = fmhip_table_apply(gone, k.data(), 33, c.data(), 1, out);
        if (st != read || (st != FMHIP_OK && st != FMHIP_ERR_INVALID_ARGUMENT)) die("a given-up x", st, read);
        if (st == FMHIP_OK) rel(out[0]); else if (out[0] != 0) die("a refused call wrote its outputs", n, 0);
        std::printf("given up: status %d\n", st);
        rel(gone);
    }
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handle keeps them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    {
        const D c0 = table(k, 3, 0, 0, 0), c1 = table(k, 3, 0, 1, 0);
        D both(c0); both.insert(both.end(), c1.begin(), c1.end());
        for (int i : { 0, 3, 5 }) {
            V out[2] = { 0, 0 };
            OK(fmhip_table_apply(derived[(size_t)i], k.data(), 33, both.data(), 2, out));
            rel(out[0]); rel(out[1]);
        }
    }
    releaser.join();
    for (V d : derived) rel(d);
    rel(stored); rel(pending);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the three outputs of one fmhip_table_apply are its three pool allocations.  Without it this
// is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const D k = knots_of(17, 0);
    const F x = data(n, k, 3);
    V hx = upload(x);
    D coef; for (int f = 0; f < 3; ++f) { const D c = table(k, f + 1, f % 2, 0, f); coef.insert(coef.end(), c.begin(), c.end()); }
    std::vector<F> want(3, F((size_t)n)); float* cols[3] = { want[0].data(), want[1].data(), want[2].data() };
    OK(fmhip_table_apply_host(x.data(), n, k.data(), 17, coef.data(), 3, cols));
    const fmhip_pool_stats_t before = stats();
    fmhip_pool_stats_t mid = before;
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out[3] = { 0, 0, 0 };
        const int st = fmhip_table_apply(hx, k.data(), 17, coef.data(), 3, out);
        if (attempt == 0) { first = st; mid = stats(); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            for (int f = 0; f < 3; ++f) {
                const F got = download(out[f], n);
                if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("a tabulated function", n, f);
                rel(out[f]);
            }
        } else if (out[0] != 0 || out[1] != 0 || out[2] != 0) die("a failed call wrote its outputs", n, 0);
        const fmhip_pool_stats_t after = stats();
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a table_apply left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(hx);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: table done\n", cycle);
        std::fflush(stdout);
    });
    if (plain) {                                                                // a device list of ONE shard is that shard's call
        const int device = 0;
        OK(fmhip_init_devices(&device, 1));
        scenario(false, true);
        OK(fmhip_shutdown());
        std::printf("a device list of one shard: checked\n");
    }
    return 0;
}
