// drive_transform.cpp — drives fmhip_transform_option through the C-ABI on the TEST-ONLY null device under the sanitizers: vectors of real
// data at sizes around the kernel's tile and group — forwards around the strike with zeros, negatives, infinities and NaNs scattered among
// them, payoff units, states with a NaN, an overflowing and an out-of-range one — 0, 1 and 2 states, tables of 1, 2, 65 and 256 nodes, every
// mask the state count allows, every combination of vector and scalar operands; every result compared bit for bit with
// fmhip_transform_option_host (the stand-in launcher of null_transform.cpp walks the groups THE KERNEL'S WAY, from the launch's argument
// block and the table's device copy); pending (fused, unflushed) operands; every argument refusal with nothing flushed, launched,
// allocated or left behind.  Twice, with a shutdown and a re-initialisation in between.  FMNULL_DEVICES=N: behind a device list of N shards
// (every shard its block); FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked about by a thread that does not own them.
// `failure`: FMHIP_TEST_FAIL_ALLOC_AT on each of the call's allocations.
// The null device computes nothing element-wise, so a pending operand is compared with what its buffer holds once it exists.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static V upload(const F& v) { V h = 0; OK(fmhip_vec_create_from_float(v.data(), (int64_t)v.size(), &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static fmhip_pool_stats_t stats() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st; }

static F data(int64_t n, double lo, double hi, unsigned seed) {
    F a((size_t)n);
    uint64_t s = 0x9e3779b97f4a7c15ull * (seed + 1);
    for (int64_t p = 0; p < n; ++p) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        a[(size_t)p] = (float)(lo + (hi - lo) * ((double)(s >> 11) * 0x1.0p-53));
    }
    return a;
}

// a table of the rule's shape: Black–Scholes' a, states that damp and turn
static std::vector<double> table(int J, int S) {
    std::vector<double> t((size_t)J * (size_t)(3 + 2 * S));
    for (int j = 0; j < J; ++j) {
        double* row = t.data() + (size_t)j * (size_t)(3 + 2 * S);
        const double x = (j + 0.5) / J, u = 60.0 * x * x, w = 120.0 * x / J;
        row[0] = u; row[1] = -0.02 * (u * u + 0.25) + std::log(w / (3.14159265358979323846 * (u * u + 0.25))); row[2] = 0.01 * u;
        for (int s = 0; s < S; ++s) { row[3 + s] = -0.5 * (u * u + 0.25) / (s + 1); row[3 + S + s] = -0.3 * u / (s + 1); }
    }
    return t;
}

// use: bit k set = operand k (forward, payoff unit, V_0, V_1) is its vector, otherwise the scalar
static void check(const std::vector<double>& t, int J, int S, const V* h, const F* host, int use, const double* scalars, double K, int mask) {
    const int64_t n = (int64_t)host[0].size();
    const int n_out = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1);
    V out[3] = { 0, 0, 0 };
    const V states[2] = { use & 4 ? h[2] : 0, use & 8 ? h[3] : 0 };
    const float* host_states[2] = { use & 4 ? host[2].data() : nullptr, use & 8 ? host[3].data() : nullptr };
    OK(fmhip_transform_option(t.data(), J, S, use & 1 ? h[0] : 0, scalars[0], S ? states : nullptr, S ? scalars + 2 : nullptr, use & 2 ? h[1] : 0, scalars[1], K, mask, out));
    std::vector<F> want((size_t)n_out, F((size_t)n));
    float* cols[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < n_out; ++f) cols[f] = want[(size_t)f].data();
    OK(fmhip_transform_option_host(t.data(), J, S, use & 1 ? host[0].data() : nullptr, scalars[0], S ? host_states : nullptr, S ? scalars + 2 : nullptr,
                                   use & 2 ? host[1].data() : nullptr, scalars[1], n, K, mask, cols));
    for (int f = 0; f < n_out; ++f) {
        int64_t size = -1; OK(fmhip_vec_size(out[f], &size));
        if (size != n) die("the size of a result", n, size);
        const F got = download(out[f], n);
        if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("a transform option value differs from the definition", n, S * 10000 + J * 100 + use * 10 + mask);
        rel(out[f]);
    }
    for (int f = n_out; f < 3; ++f) if (out[f] != 0) die("more outputs than the mask has bits", n, mask);
}

static void refusals(V x, V shorter, int64_t n) {
    const fmhip_pool_stats_t before = stats();
    V out[3] = { 0, 0, 0 };
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const std::vector<double> t = table(8, 1), t0 = table(8, 0);
    std::vector<double> bad = t; bad[11] = inf;
    std::vector<double> worse = t; worse[39] = nan;
    const V none[2] = { 0, 0 }, mismatched[2] = { shorter, 0 }, wild[2] = { x + 1000000, 0 };
    const double sc[2] = { 0.04, 0.0 };
    EXPECT(fmhip_transform_option(t.data(), 0, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 257, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, -1, x, 0, none, sc, 0, 1.0, 100.0, 3, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 3, x, 0, none, sc, 0, 1.0, 100.0, 3, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 8, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t0.data(), 8, 0, x, 0, nullptr, nullptr, 0, 1.0, 100.0, 4, out), FMHIP_ERR_INVALID_ARGUMENT);      // the state delta without a state
    EXPECT(fmhip_transform_option(nullptr, 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, nullptr, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, none, nullptr, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(bad.data(), 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(worse.data(), 8, 1, x, 0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, 0, 100.0, none, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);            // no vector among the operands
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, none, sc, 0, 1.0, nan, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, mismatched, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_transform_option(t.data(), 8, 1, x, 0, wild, sc, 0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_HANDLE);
    // the host-only call
    F hx((size_t)4, 100.0f), ho((size_t)4); float* col[1] = { ho.data() }; float* hole[1] = { nullptr };
    const float* no_states[1] = { nullptr };
    EXPECT(fmhip_transform_option_host(t.data(), 8, 1, hx.data(), 0, no_states, sc, nullptr, 1.0, 4, 100.0, 1, hole), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option_host(t.data(), 8, 1, hx.data(), 0, no_states, sc, nullptr, 1.0, 0, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option_host(t.data(), 8, 1, hx.data(), 0, no_states, sc, nullptr, 1.0, 4, 100.0, 9, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_transform_option_host(t.data(), 8, 1, nullptr, 100.0, no_states, sc, nullptr, 1.0, 4, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    if (out[0] != 0 || out[1] != 0 || out[2] != 0) die("a refused call wrote its outputs", n, 0);
    const fmhip_pool_stats_t after = stats();
    if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    if (after.n_alloc_hits + after.n_alloc_misses != before.n_alloc_hits + before.n_alloc_misses) die("a refused call allocated", n, 0);
    if (after.n_kernel_launches != before.n_kernel_launches) die("a refused call launched", n, 0);
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099, 100003 };
    const int counts[] = { 1, 2, 65, 256 };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int turn = 0;
    for (int64_t n : sizes) {
        F f = data(n, 40.0, 180.0, (unsigned)n + 1), w = data(n, 0.5, 1.5, (unsigned)n + 3), a = data(n, 0.0, 0.3, (unsigned)n + 5), b = data(n, 0.0, 0.1, (unsigned)n + 7);
        const float edge[] = { 0.0f, -0.0f, -3.0f, inf, -inf, nan, std::numeric_limits<float>::denorm_min() };
        for (int64_t p = 5; p < n; p += 53) f[(size_t)p] = edge[(size_t)(p / 53) % 7];
        if (n > 40) { w[37] = nan; a[38] = nan; a[39] = -3e38f; a[40] = 3e38f; }
        if (n > 60) { w[41] = 0.0f; w[43] = -1.0f; b[44] = nan; b[45] = inf; }
        const F host[4] = { f, w, a, b };
        const V h[4] = { upload(f), upload(w), upload(a), upload(b) };
        const int64_t live = stats().n_live_vectors;
        const double scalars[4] = { 104.5, 0.9, 0.03, 0.015 };
        for (int S = 0; S <= 2; ++S) {
            const int J = n > 5000 ? 2 : counts[(size_t)(turn % 4)];
            const std::vector<double> t = table(J, S);
            for (int use = 1; use < (4 << S); ++use) {
                const int mask = S ? 1 + (turn++ % 7) : 1 + (turn++ % 3);
                auto run = [&] { check(t, J, S, h, host, use, scalars, 100.0, mask); };
                if (thread_engines && use % 2 == 0) { std::thread asker(run); asker.join(); }       // a thread that does not own the vectors
                else run();
            }
            if (n == 65 || n == 4099) for (int mask = 1; mask < (S ? 8 : 4); ++mask) { check(t, J, S, h, host, (4 << S) - 1, scalars, 100.0, mask); check(t, J, S, h, host, 1, scalars, 0.0, mask); }
        }
        if (stats().n_live_vectors != live) die("the calls left vectors behind", n, 0);
        if (n == 4099) { V shorter = upload(F(7, 1.0f)); refusals(h[0], shorter, n); rel(shorter); }
        for (V v : h) rel(v);
    }
    // pending (fused, unflushed) operands: the results against what the vectors hold once they exist
    const int64_t n = 2051;
    const F base = data(n, 50.0, 150.0, 9);
    V stored = upload(base);
    V pending = 0, pending2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 3.0, &pending));              // forwards
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 0.001, &pending2));          // variances
    {
        const std::vector<double> t = table(64, 1);
        V out[3] = { 0, 0, 0 };
        const V states[1] = { pending2 }; const double sc[1] = { 0.0 };
        OK(fmhip_transform_option(t.data(), 64, 1, pending, 0, states, sc, 0, 0.5, 100.0, 7, out));      // two pending operands: one flush
        const F fw = download(pending, n), va = download(pending2, n);
        F w0((size_t)n), w1((size_t)n), w2((size_t)n); float* c3[3] = { w0.data(), w1.data(), w2.data() };
        const float* hs[1] = { va.data() };
        OK(fmhip_transform_option_host(t.data(), 64, 1, fw.data(), 0, hs, sc, nullptr, 0.5, n, 100.0, 7, c3));
        for (int f = 0; f < 3; ++f) { if (std::memcmp(download(out[f], n).data(), c3[f], (size_t)n * 4) != 0) die("a transform option value of pending vectors", n, f); rel(out[f]); }
    }
    rel(stored); rel(pending); rel(pending2);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the three outputs of one call are its pool allocations.  Without it this is the counting
// run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const F f = data(n, 50.0, 150.0, 3), a = data(n, 0.0, 0.3, 4);
    const std::vector<double> t = table(16, 1);
    V hf = upload(f), ha = upload(a);
    std::vector<F> want(3, F((size_t)n)); float* cols[3] = { want[0].data(), want[1].data(), want[2].data() };
    const float* hs[1] = { a.data() }; const double sc[1] = { 0.0 };
    OK(fmhip_transform_option_host(t.data(), 16, 1, f.data(), 0, hs, sc, nullptr, 0.9, n, 100.0, 7, cols));
    const fmhip_pool_stats_t before = stats();
    fmhip_pool_stats_t mid = before;
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out[3] = { 0, 0, 0 };
        const V states[1] = { ha };
        const int st = fmhip_transform_option(t.data(), 16, 1, hf, 0, states, sc, 0, 0.9, 100.0, 7, out);
        if (attempt == 0) { first = st; mid = stats(); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            for (int o = 0; o < 3; ++o) {
                const F got = download(out[o], n);
                if (std::memcmp(got.data(), want[(size_t)o].data(), (size_t)n * 4) != 0) die("a result", n, o);
                rel(out[o]);
            }
        } else if (out[0] != 0 || out[1] != 0 || out[2] != 0) die("a failed call wrote its outputs", n, 0);
        const fmhip_pool_stats_t after = stats();
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(hf); rel(ha);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: transform option done\n", cycle);
        std::fflush(stdout);
    });
    return 0;
}
