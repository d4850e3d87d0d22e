// drive_implied_volatility_absent.cpp — a build of the engine WITHOUT the launcher of implied_volatility_kernel.hip (no stand-in for it is
// linked: the weak reference stays null) on the TEST-ONLY null device: fmhip_implied_volatility answers FMHIP_ERR_UNSUPPORTED — after its
// argument checks, which still come first — and never falls back; the host-only call needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101) * 0.125f + 1.0f;
        fmhip_vec v = 0, out[3] = { 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_implied_volatility(2, v, 0.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_implied_volatility(FMHIP_FORMULA_BACHELIER, 0, 1.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_implied_volatility(FMHIP_FORMULA_BACHELIER, v, 0.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 7, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_implied_volatility(FMHIP_FORMULA_BLACK_SCHOLES, 0, 1.0, v, 0.0, v, 0.0, 1.0, 1.0, FMHIP_IMPLIED_D_FORWARD, out), FMHIP_ERR_UNSUPPORTED);
        if (out[0] != 0 || out[1] != 0 || out[2] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> sigma((size_t)n, -1.0f), d_price((size_t)n, -1.0f);
        float* cols[2] = { sigma.data(), d_price.data() };
        // at the money under Bachelier the root is price·√(2π)/√T: the definition needs no kernel
        OK(fmhip_implied_volatility_host(FMHIP_FORMULA_BACHELIER, a.data(), 0.0, nullptr, 100.0, nullptr, 1.0, n, 4.0, 100.0, FMHIP_IMPLIED_VOLATILITY | FMHIP_IMPLIED_D_PRICE, cols));
        for (int64_t p = 0; p < n; ++p) {
            const double want = (double)a[(size_t)p] * 2.5066282746310002 / 2.0;
            if (!(sigma[(size_t)p] >= (float)(want * 0.999999) && sigma[(size_t)p] <= (float)(want * 1.000001) && d_price[(size_t)p] > 1.25f && d_price[(size_t)p] < 1.26f)) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)p); std::abort(); }
        }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: implied volatility absent done\n", cycle);
        std::fflush(stdout);
    });
}
