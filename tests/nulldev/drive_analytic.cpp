// drive_analytic.cpp — drives fmhip_function_apply and fmhip_option_formula through the C-ABI on the TEST-ONLY null device under the
// sanitizers: vectors of real data at sizes around the kernels' tile and group, every kind alone, the pair, all three with a repeat; both
// models, every mask, every combination of vector and scalar operands, degenerate and NaN elements among live ones, T = 0; every result
// compared bit for bit with fmhip_function_apply_host / fmhip_option_formula_host (the stand-in launchers of null_analytic.cpp walk the groups
// THE KERNELS' WAY, from the launch's argument block); pending (fused, unflushed) operands, a given-up operand, a second thread releasing
// the inputs of pending operands during the calls, every argument refusal with nothing flushed, launched or left behind.  Twice, with a
// shutdown and a re-initialisation in between.  FMNULL_DEVICES=N: behind a device list of N shards (every shard its block);
// FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked about by a thread that does not own them.
// `failure function|formula`: FMHIP_TEST_FAIL_ALLOC_AT on each of the output allocations.
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

// lo … hi, with the edge inputs scattered in
static F data(int64_t n, double lo, double hi, unsigned seed, bool edges = true) {
    F a((size_t)n);
    uint64_t s = 0x9e3779b97f4a7c15ull * (seed + 1);
    for (int64_t p = 0; p < n; ++p) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        a[(size_t)p] = (float)(lo + (hi - lo) * ((double)(s >> 11) * 0x1.0p-53));
    }
    const float edge[] = { 0.0f, -0.0f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(),
                           std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), 1.0f, 1.0f - 0x1.0p-24f, -1.0f, 2.0f };
    if (edges) for (size_t e = 0; e < sizeof edge / sizeof *edge && (int64_t)e < n; ++e) a[(size_t)((e * 977) % (size_t)n)] = edge[e];
    return a;
}

static void check_functions(V hx, const F& x, const int* kinds, int T) {
    const int64_t n = (int64_t)x.size();
    V out[4] = { 0, 0, 0, 0 };
    OK(fmhip_function_apply(hx, kinds, T, out));
    std::vector<F> want((size_t)T, F((size_t)n));
    float* cols[4] = { nullptr, nullptr, nullptr, nullptr };
    for (int f = 0; f < T; ++f) cols[f] = want[(size_t)f].data();
    OK(fmhip_function_apply_host(x.data(), n, kinds, T, cols));
    for (int f = 0; f < T; ++f) {
        int64_t size = -1; OK(fmhip_vec_size(out[f], &size));
        if (size != n) die("the size of a result", n, size);
        const F got = download(out[f], n);
        if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("a named function differs from the definition", n, kinds[f]);
        rel(out[f]);
    }
}

// use: bit k set = operand k is its vector, otherwise the scalar
static void check_formula(int model, const V* h, const F* host, int use, const double* scalars, double T, double K, int mask) {
    const int64_t n = (int64_t)host[0].size();
    const int n_out = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1);
    V out[3] = { 0, 0, 0 };
    OK(fmhip_option_formula(model, use & 1 ? h[0] : 0, scalars[0], use & 2 ? h[1] : 0, scalars[1], use & 4 ? h[2] : 0, scalars[2], T, K, mask, out));
    std::vector<F> want((size_t)n_out, F((size_t)n));
    float* cols[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < n_out; ++f) cols[f] = want[(size_t)f].data();
    OK(fmhip_option_formula_host(model, use & 1 ? host[0].data() : nullptr, scalars[0], use & 2 ? host[1].data() : nullptr, scalars[1], use & 4 ? host[2].data() : nullptr, scalars[2], n, T, K, mask, cols));
    for (int f = 0; f < n_out; ++f) {
        int64_t size = -1; OK(fmhip_vec_size(out[f], &size));
        if (size != n) die("the size of a result", n, size);
        const F got = download(out[f], n);
        if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("an option formula differs from the definition", n, model * 1000 + use * 10 + mask);
        rel(out[f]);
    }
    for (int f = n_out; f < 3; ++f) if (out[f] != 0) die("more outputs than the mask has bits", n, mask);
}

static void refusals(V x, V shorter, int64_t n) {
    const fmhip_pool_stats_t before = stats();
    V out[4] = { 0, 0, 0, 0 };
    const int kinds[5] = { 0, 1, 2, 0, 1 }, unknown[1] = { 3 }, negative[1] = { -1 };
    EXPECT(fmhip_function_apply(0, kinds, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, nullptr, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, kinds, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, kinds, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, kinds, 5, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, unknown, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x, negative, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply(x + 1000000, kinds, 1, out), FMHIP_ERR_INVALID_HANDLE);
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    EXPECT(fmhip_option_formula(2, x, 0, 0, 0.2, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(-1, x, 0, 0, 0.2, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, 0, 100.0, 0, 0.2, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);      // no vector among the operands
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, -1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, nan, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, inf, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, 1.0, nan, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, 1.0, inf, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, 1.0, 100.0, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, 1.0, 100.0, 8, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, 0, 0.2, 0, 1, 1.0, 100.0, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula(0, x, 0, shorter, 0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_option_formula(0, x, 0, x + 1000000, 0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_HANDLE);
    // the host-only calls
    F hx((size_t)4, 0.5f), ho((size_t)4); float* col[1] = { ho.data() }; float* none[1] = { nullptr };
    EXPECT(fmhip_function_apply_host(nullptr, 4, kinds, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply_host(hx.data(), 0, kinds, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply_host(hx.data(), 4, kinds, 1, none), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_function_apply_host(hx.data(), 4, unknown, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula_host(0, hx.data(), 0, nullptr, 0.2, nullptr, 1, 4, 1.0, 100.0, 1, none), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula_host(0, hx.data(), 0, nullptr, 0.2, nullptr, 1, 4, -1.0, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_option_formula_host(0, hx.data(), 0, nullptr, 0.2, nullptr, 1, 0, 1.0, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    if (out[0] != 0 || out[1] != 0 || out[2] != 0 || out[3] != 0) die("a refused call wrote its outputs", n, 0);
    const fmhip_pool_stats_t after = stats();
    if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    if (after.n_alloc_hits + after.n_alloc_misses != before.n_alloc_hits + before.n_alloc_misses) die("a refused call allocated", n, 0);
    if (after.n_kernel_launches != before.n_kernel_launches) die("a refused call launched", n, 0);
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099, 100003 };
    const int kind_sets[][4] = { { 0, 0, 0, 0 }, { 1, 0, 0, 0 }, { 2, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 1, 2, 0 }, { 2, 1, 0, 2 } };
    const int kind_counts[] = { 1, 1, 1, 2, 3, 4 };
    int turn = 0;
    for (int64_t n : sizes) {
        const F x = data(n, -15.0, 15.0, (unsigned)n), u = data(n, 0.0, 1.0, (unsigned)n + 7);
        V hx = upload(x), hu = upload(u);
        const int64_t live = stats().n_live_vectors;
        for (int s = 0; s < 6; ++s) {
            auto run = [&] { check_functions(s % 2 ? hu : hx, s % 2 ? u : x, kind_sets[s], kind_counts[s]); };
            if (thread_engines && s % 2 == 0) { std::thread asker(run); asker.join(); }       // a thread that does not own x
            else run();
        }
        // the formulas: forwards around the strike with zeros, negatives and the edge inputs, volatilities with zeros, units with a NaN
        F f = data(n, 40.0, 180.0, (unsigned)n + 1), v = data(n, 0.01, 0.8, (unsigned)n + 2, false), w = data(n, 0.5, 1.5, (unsigned)n + 3, false);
        for (int64_t p = 0; p < n; p += 11) v[(size_t)p] = p % 22 ? 0.0f : -0.1f;
        if (n > 40) w[37] = std::numeric_limits<float>::quiet_NaN();
        const F host[3] = { f, v, w };
        const V h[3] = { upload(f), upload(v), upload(w) };
        for (int model = 0; model < 2; ++model) {
            const double scale = model == 1 ? 100.0 : 1.0;
            F vs = v; for (float& e : vs) e *= (float)scale;
            const V hv = model == 1 ? upload(vs) : h[1];
            const F host_m[3] = { f, vs, w };
            const V h_m[3] = { h[0], hv, h[2] };
            const double scalars[3] = { 104.5, 0.3 * scale, 0.9 };
            for (int use = 1; use < 8; ++use) {
                const int mask = 1 + (turn++ % 7);
                auto run = [&] { check_formula(model, h_m, host_m, use, scalars, n % 2 ? 1.5 : 0.25, 100.0, mask); };
                if (thread_engines && use % 2 == 0) { std::thread asker(run); asker.join(); }
                else run();
            }
            if (n == 65 || n == 4099) for (int mask = 1; mask < 8; ++mask) { check_formula(model, h_m, host_m, 7, scalars, 2.0, 100.0, mask); check_formula(model, h_m, host_m, 5, scalars, 0.0, 100.0, mask); }
            if (model == 1) rel(hv);
        }
        for (V g : h) rel(g);
        if (stats().n_live_vectors != live) die("the calls left vectors behind", n, 0);
        if (n == 4099) { V shorter = upload(F(7, 1.0f)); refusals(hx, shorter, n); rel(shorter); }
        rel(hx); rel(hu);
    }
    // pending (fused, unflushed) operands: the results against what the vectors hold once they exist
    const int64_t n = 2051;
    const F base = data(n, 50.0, 150.0, 9, false);
    V stored = upload(base);
    V pending = 0, pending2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 0.01, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 3.0, &pending2));
    {
        const int kinds[2] = { 0, 1 };
        V out[3] = { 0, 0, 0 };
        OK(fmhip_function_apply(pending, kinds, 2, out));
        const F x = download(pending, n);
        F want0((size_t)n), want1((size_t)n); float* cols[2] = { want0.data(), want1.data() };
        OK(fmhip_function_apply_host(x.data(), n, kinds, 2, cols));
        if (std::memcmp(download(out[0], n).data(), want0.data(), (size_t)n * 4) != 0 || std::memcmp(download(out[1], n).data(), want1.data(), (size_t)n * 4) != 0) die("a named function of a pending vector", n, 0);
        rel(out[0]); rel(out[1]);
        OK(fmhip_option_formula(FMHIP_FORMULA_BLACK_SCHOLES, pending2, 0, pending, 0, 0, 0.5, 1.0, 100.0, 7, out));      // two pending operands: one flush
        const F fw = download(pending2, n);
        F w0((size_t)n), w1((size_t)n), w2((size_t)n); float* c3[3] = { w0.data(), w1.data(), w2.data() };
        OK(fmhip_option_formula_host(FMHIP_FORMULA_BLACK_SCHOLES, fw.data(), 0, x.data(), 0, nullptr, 0.5, n, 1.0, 100.0, 7, c3));
        for (int f = 0; f < 3; ++f) { if (std::memcmp(download(out[f], n).data(), c3[f], (size_t)n * 4) != 0) die("an option formula of pending vectors", n, f); rel(out[f]); }
    }
    // a given-up operand whose values the engine has not kept: the error a read of it is
    if (!sharded && !thread_engines) {
        V gone = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 5.0, &gone));
        OK(fmhip_vec_give_up_values(&gone, 1));
        fmhip_ticket ticket = 0; fmhip_moments mo;
        OK(fmhip_reduce_moments_batch_begin(&gone, 1, nullptr, &ticket));
        OK(fmhip_reduce_moments_batch_end(ticket, &mo, 1));
        F h((size_t)n);
        const int read = fmhip_vec_read_float(gone, h.data(), n);
        const int kinds[1] = { 0 };
        V out[3] = { 0, 0, 0 };
        const int st = fmhip_function_apply(gone, kinds, 1, out);
        if (st != read || (st != FMHIP_OK && st != FMHIP_ERR_INVALID_ARGUMENT)) die("a given-up x", st, read);
        if (st == FMHIP_OK) rel(out[0]); else if (out[0] != 0) die("a refused call wrote its outputs", n, 0);
        out[0] = 0;
        const int st2 = fmhip_option_formula(FMHIP_FORMULA_BACHELIER, stored, 0, gone, 0, 0, 1.0, 1.0, 100.0, 3, out);
        if (st2 != read) die("a given-up volatility", st2, read);
        if (st2 == FMHIP_OK) { rel(out[0]); rel(out[1]); } else if (out[0] != 0 || out[1] != 0) die("a refused call wrote its outputs", n, 1);
        std::printf("given up: status %d\n", st);
        rel(gone);
    }
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 0.02, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    {
        const int kinds[2] = { 0, 1 };
        for (int i : { 0, 3, 5 }) {
            V out[3] = { 0, 0, 0 };
            OK(fmhip_function_apply(derived[(size_t)i], kinds, 2, out));
            rel(out[0]); rel(out[1]);
            OK(fmhip_option_formula(FMHIP_FORMULA_BACHELIER, stored, 0, derived[(size_t)i], 0, derived[(size_t)((i + 1) % 6)], 0, 1.0, 100.0, 5, out));
            rel(out[0]); rel(out[1]);
        }
    }
    releaser.join();
    for (V d : derived) rel(d);
    rel(stored); rel(pending); rel(pending2);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the three outputs of one call are its three pool allocations.  Without it this is the
// counting run that says where they are.
static int failure(bool formula) {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const F x = formula ? data(n, 50.0, 150.0, 3) : data(n, -6.0, 6.0, 3), s = data(n, 0.05, 0.5, 4, false);
    V hx = upload(x), hs = upload(s);
    const int kinds[3] = { 0, 1, 2 };
    std::vector<F> want(3, F((size_t)n)); float* cols[3] = { want[0].data(), want[1].data(), want[2].data() };
    if (formula) OK(fmhip_option_formula_host(FMHIP_FORMULA_BLACK_SCHOLES, x.data(), 0, s.data(), 0, nullptr, 0.9, n, 2.0, 100.0, 7, cols));
    else OK(fmhip_function_apply_host(x.data(), n, kinds, 3, cols));
    const fmhip_pool_stats_t before = stats();
    fmhip_pool_stats_t mid = before;
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out[3] = { 0, 0, 0 };
        const int st = formula ? fmhip_option_formula(FMHIP_FORMULA_BLACK_SCHOLES, hx, 0, hs, 0, 0, 0.9, 2.0, 100.0, 7, out) : fmhip_function_apply(hx, kinds, 3, out);
        if (attempt == 0) { first = st; mid = stats(); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            for (int f = 0; f < 3; ++f) {
                const F got = download(out[f], n);
                if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("a result", n, f);
                rel(out[f]);
            }
        } else if (out[0] != 0 || out[1] != 0 || out[2] != 0) die("a failed call wrote its outputs", n, 0);
        const fmhip_pool_stats_t after = stats();
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(hx); rel(hs);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 2 && std::string(argv[1]) == "failure") return failure(std::string(argv[2]) == "formula");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: analytic done\n", cycle);
        std::fflush(stdout);
    });
    return 0;
}
