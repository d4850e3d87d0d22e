// drive_implied_volatility.cpp — drives fmhip_implied_volatility through the C-ABI on the TEST-ONLY null device under the sanitizers:
// vectors of real data at sizes around the kernel's tile and group — prices made by fmhip_option_formula_host from volatilities, with
// prices below the intrinsic value, above the upper bound, at either, zeros, negatives, infinities and NaNs scattered among them — both
// models, every mask, every combination of vector and scalar operands, T = 0; every result compared bit for bit with
// fmhip_implied_volatility_host (the stand-in launcher of null_implied_volatility.cpp walks the groups THE KERNEL'S WAY, from the launch's
// argument block); pending (fused, unflushed) operands, a given-up operand, a second thread releasing the inputs of pending operands
// during the calls, every argument refusal with nothing flushed, launched or left behind.  Twice, with a shutdown and a re-initialisation
// in between.  FMNULL_DEVICES=N: behind a device list of N shards (every shard its block); FMNULL_THREAD_ENGINES=1: an engine per caller
// thread, the vectors asked about by a thread that does not own them.
// `failure`: FMHIP_TEST_FAIL_ALLOC_AT on each of the output allocations.
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

// prices of model at (forward, unit) and volatilities in [0.05, 0.8] (times scale), with the edge prices scattered in
static F prices(int model, const F& forward, const F& unit, double T, double K, unsigned seed) {
    const int64_t n = (int64_t)forward.size();
    F sigma = data(n, 0.05, 0.8, seed), value((size_t)n);
    if (model == FMHIP_FORMULA_BACHELIER) for (float& e : sigma) e *= 100.0f;
    float* col[1] = { value.data() };
    OK(fmhip_option_formula_host(model, forward.data(), 0, sigma.data(), 0, unit.data(), 0, n, T > 0 ? T : 1.0, K, FMHIP_FORMULA_VALUE, col));
    const float inf = std::numeric_limits<float>::infinity();
    for (int64_t p = 0; p < n; p += 7) {
        const float intrinsic = unit[(size_t)p] * std::fmax(forward[(size_t)p] - (float)K, 0.0f);
        const float edge[] = { intrinsic, intrinsic * 0.5f - 1.0f, unit[(size_t)p] * forward[(size_t)p], unit[(size_t)p] * forward[(size_t)p] * 2.0f, 0.0f, -0.0f, inf, -inf,
                               std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::denorm_min(), std::nextafter(intrinsic, inf) };
        value[(size_t)p] = edge[(size_t)(p / 7) % (sizeof edge / sizeof *edge)];
    }
    return value;
}

// use: bit k set = operand k is its vector, otherwise the scalar
static void check(int model, const V* h, const F* host, int use, const double* scalars, double T, double K, int mask) {
    const int64_t n = (int64_t)host[0].size();
    const int n_out = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1);
    V out[3] = { 0, 0, 0 };
    OK(fmhip_implied_volatility(model, use & 1 ? h[0] : 0, scalars[0], use & 2 ? h[1] : 0, scalars[1], use & 4 ? h[2] : 0, scalars[2], T, K, mask, out));
    std::vector<F> want((size_t)n_out, F((size_t)n));
    float* cols[3] = { nullptr, nullptr, nullptr };
    for (int f = 0; f < n_out; ++f) cols[f] = want[(size_t)f].data();
    OK(fmhip_implied_volatility_host(model, use & 1 ? host[0].data() : nullptr, scalars[0], use & 2 ? host[1].data() : nullptr, scalars[1], use & 4 ? host[2].data() : nullptr, scalars[2], n, T, K, mask, cols));
    for (int f = 0; f < n_out; ++f) {
        int64_t size = -1; OK(fmhip_vec_size(out[f], &size));
        if (size != n) die("the size of a result", n, size);
        const F got = download(out[f], n);
        if (std::memcmp(got.data(), want[(size_t)f].data(), (size_t)n * 4) != 0) die("an implied volatility differs from the definition", n, model * 1000 + use * 10 + mask);
        rel(out[f]);
    }
    for (int f = n_out; f < 3; ++f) if (out[f] != 0) die("more outputs than the mask has bits", n, mask);
}

static void refusals(V x, V shorter, int64_t n) {
    const fmhip_pool_stats_t before = stats();
    V out[3] = { 0, 0, 0 };
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    EXPECT(fmhip_implied_volatility(2, x, 0, 0, 100.0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(-1, x, 0, 0, 100.0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, 0, 8.0, 0, 100.0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);      // no vector among the operands
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, -1.0, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, nan, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, inf, 100.0, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, 1.0, nan, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, 1.0, inf, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, 1.0, 100.0, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, 1.0, 100.0, 8, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, 0, 100.0, 0, 1, 1.0, 100.0, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility(0, x, 0, shorter, 0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_implied_volatility(0, x, 0, x + 1000000, 0, 0, 1, 1.0, 100.0, 1, out), FMHIP_ERR_INVALID_HANDLE);
    // the host-only call
    F hx((size_t)4, 8.0f), ho((size_t)4); float* col[1] = { ho.data() }; float* none[1] = { nullptr };
    EXPECT(fmhip_implied_volatility_host(0, hx.data(), 0, nullptr, 100.0, nullptr, 1, 4, 1.0, 100.0, 1, none), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility_host(0, hx.data(), 0, nullptr, 100.0, nullptr, 1, 4, -1.0, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility_host(0, hx.data(), 0, nullptr, 100.0, nullptr, 1, 0, 1.0, 100.0, 1, col), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_implied_volatility_host(0, hx.data(), 0, nullptr, 100.0, nullptr, 1, 4, 1.0, 100.0, 9, col), FMHIP_ERR_INVALID_ARGUMENT);
    if (out[0] != 0 || out[1] != 0 || out[2] != 0) die("a refused call wrote its outputs", n, 0);
    const fmhip_pool_stats_t after = stats();
    if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a refused call left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    if (after.n_alloc_hits + after.n_alloc_misses != before.n_alloc_hits + before.n_alloc_misses) die("a refused call allocated", n, 0);
    if (after.n_kernel_launches != before.n_kernel_launches) die("a refused call launched", n, 0);
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t sizes[] = { 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4099, 100003 };
    int turn = 0;
    for (int64_t n : sizes) {
        F f = data(n, 40.0, 180.0, (unsigned)n + 1), w = data(n, 0.5, 1.5, (unsigned)n + 3);
        for (int64_t p = 5; p < n; p += 53) f[(size_t)p] = p % 2 ? 0.0f : -3.0f;
        if (n > 40) w[37] = std::numeric_limits<float>::quiet_NaN();
        if (n > 60) { w[41] = 0.0f; w[43] = -1.0f; }
        const V hf = upload(f), hw = upload(w);
        const int64_t live = stats().n_live_vectors;
        for (int model = 0; model < 2; ++model) {
            const double T = n % 2 ? 1.5 : 0.25, K = 100.0;
            const F c = prices(model, f, w, T, K, (unsigned)n + 5);
            const V hc = upload(c);
            const F host[3] = { c, f, w };
            const V h[3] = { hc, hf, hw };
            const double scalars[3] = { 9.5, 104.5, 0.9 };
            for (int use = 1; use < 8; ++use) {
                const int mask = 1 + (turn++ % 7);
                auto run = [&] { check(model, h, host, use, scalars, T, K, mask); };
                if (thread_engines && use % 2 == 0) { std::thread asker(run); asker.join(); }       // a thread that does not own the vectors
                else run();
            }
            if (n == 65 || n == 4099) for (int mask = 1; mask < 8; ++mask) { check(model, h, host, 7, scalars, 2.0, K, mask); check(model, h, host, 5, scalars, 0.0, K, mask); }
            rel(hc);
        }
        if (stats().n_live_vectors != live) die("the calls left vectors behind", n, 0);
        if (n == 4099) { V shorter = upload(F(7, 1.0f)); refusals(hf, shorter, n); rel(shorter); }
        rel(hf); rel(hw);
    }
    // pending (fused, unflushed) operands: the results against what the vectors hold once they exist
    const int64_t n = 2051;
    const F base = data(n, 50.0, 150.0, 9);
    V stored = upload(base);
    V pending = 0, pending2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 0.2, &pending));            // prices
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 3.0, &pending2));            // forwards
    {
        V out[3] = { 0, 0, 0 };
        OK(fmhip_implied_volatility(FMHIP_FORMULA_BLACK_SCHOLES, pending, 0, pending2, 0, 0, 0.5, 1.0, 100.0, 7, out));      // two pending operands: one flush
        const F c = download(pending, n), fw = download(pending2, n);
        F w0((size_t)n), w1((size_t)n), w2((size_t)n); float* c3[3] = { w0.data(), w1.data(), w2.data() };
        OK(fmhip_implied_volatility_host(FMHIP_FORMULA_BLACK_SCHOLES, c.data(), 0, fw.data(), 0, nullptr, 0.5, n, 1.0, 100.0, 7, c3));
        for (int f = 0; f < 3; ++f) { if (std::memcmp(download(out[f], n).data(), c3[f], (size_t)n * 4) != 0) die("an implied volatility of pending vectors", n, f); rel(out[f]); }
    }
    // a given-up operand whose values the engine has not kept: the error a read of it is
    if (!sharded && !thread_engines) {
        V gone = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 0.1, &gone));
        OK(fmhip_vec_give_up_values(&gone, 1));
        fmhip_ticket ticket = 0; fmhip_moments mo;
        OK(fmhip_reduce_moments_batch_begin(&gone, 1, nullptr, &ticket));
        OK(fmhip_reduce_moments_batch_end(ticket, &mo, 1));
        F h((size_t)n);
        const int read = fmhip_vec_read_float(gone, h.data(), n);
        V out[3] = { 0, 0, 0 };
        const int st = fmhip_implied_volatility(FMHIP_FORMULA_BACHELIER, gone, 0, stored, 0, 0, 1.0, 1.0, 100.0, 3, out);
        if (st != read || (st != FMHIP_OK && st != FMHIP_ERR_INVALID_ARGUMENT)) die("a given-up price", st, read);
        if (st == FMHIP_OK) { rel(out[0]); rel(out[1]); } else if (out[0] != 0 || out[1] != 0) die("a refused call wrote its outputs", n, 1);
        std::printf("given up: status %d\n", st);
        rel(gone);
    }
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 0.3, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    for (int i : { 0, 3, 5 }) {
        V out[3] = { 0, 0, 0 };
        OK(fmhip_implied_volatility(FMHIP_FORMULA_BACHELIER, derived[(size_t)i], 0, stored, 0, derived[(size_t)((i + 1) % 6)], 0, 1.0, 100.0, 5, out));
        rel(out[0]); rel(out[1]);
    }
    releaser.join();
    for (V d : derived) rel(d);
    rel(stored); rel(pending); rel(pending2);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the three outputs of one call are its three pool allocations.  Without it this is the
// counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const F f = data(n, 50.0, 150.0, 3), w = data(n, 0.5, 1.5, 4), c = prices(FMHIP_FORMULA_BLACK_SCHOLES, f, w, 2.0, 100.0, 5);
    V hc = upload(c), hf = upload(f);
    std::vector<F> want(3, F((size_t)n)); float* cols[3] = { want[0].data(), want[1].data(), want[2].data() };
    OK(fmhip_implied_volatility_host(FMHIP_FORMULA_BLACK_SCHOLES, c.data(), 0, f.data(), 0, nullptr, 0.9, n, 2.0, 100.0, 7, cols));
    const fmhip_pool_stats_t before = stats();
    fmhip_pool_stats_t mid = before;
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out[3] = { 0, 0, 0 };
        const int st = fmhip_implied_volatility(FMHIP_FORMULA_BLACK_SCHOLES, hc, 0, hf, 0, 0, 0.9, 2.0, 100.0, 7, out);
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
    rel(hc); rel(hf);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: implied volatility done\n", cycle);
        std::fflush(stdout);
    });
    return 0;
}
