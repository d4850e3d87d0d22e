// drive_analytic_absent.cpp — a build of the engine WITHOUT the launchers of analytic_kernel.hip (no stand-in for them is linked: the weak
// references stay null) on the TEST-ONLY null device: fmhip_function_apply and fmhip_option_formula answer FMHIP_ERR_UNSUPPORTED — after
// their argument checks, which still come first — and never fall back; the host-only calls need no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101) * 0.125f - 6.0f;
        fmhip_vec v = 0, out[4] = { 0, 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        const int kinds[2] = { FMHIP_FN_NORMAL_CDF, FMHIP_FN_NORMAL_DENSITY }, bad[1] = { 7 };
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_function_apply(v, bad, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_function_apply(v, kinds, 5, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_function_apply(v, kinds, 1, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_function_apply(v, kinds, 2, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_option_formula(2, v, 0.0, 0, 0.2, 0, 1.0, 1.0, 1.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_option_formula(FMHIP_FORMULA_BACHELIER, 0, 1.0, 0, 0.2, 0, 1.0, 1.0, 1.0, 7, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_option_formula(FMHIP_FORMULA_BACHELIER, v, 0.0, 0, 0.2, 0, 1.0, 1.0, 1.0, 7, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_option_formula(FMHIP_FORMULA_BLACK_SCHOLES, 0, 1.0, v, 0.0, v, 0.0, 1.0, 1.0, FMHIP_FORMULA_VEGA, out), FMHIP_ERR_UNSUPPORTED);
        if (out[0] != 0 || out[1] != 0 || out[2] != 0 || out[3] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> cdf((size_t)n, -1.0f), density((size_t)n, -1.0f);
        float* cols[2] = { cdf.data(), density.data() };
        OK(fmhip_function_apply_host(a.data(), n, kinds, 2, cols));
        for (int64_t p = 0; p < n; ++p)
            if (!(cdf[(size_t)p] >= 0.0f && cdf[(size_t)p] <= 1.0f && density[(size_t)p] >= 0.0f && (a[(size_t)p] != 0.0f || cdf[(size_t)p] == 0.5f))) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)p); std::abort(); }
        OK(fmhip_option_formula_host(FMHIP_FORMULA_BACHELIER, a.data(), 0.0, nullptr, 0.0, nullptr, 2.0, n, 1.0, 1.0, FMHIP_FORMULA_VALUE | FMHIP_FORMULA_DELTA, cols));
        for (int64_t p = 0; p < n; ++p)                                        // volatility 0: the limit, exact on this dyadic data
            if (cdf[(size_t)p] != 2.0f * (a[(size_t)p] > 1.0f ? a[(size_t)p] - 1.0f : 0.0f) || density[(size_t)p] != (a[(size_t)p] > 1.0f ? 2.0f : 0.0f)) { std::fprintf(stderr, "the limit is off at %lld\n", (long long)p); std::abort(); }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: analytic absent done\n", cycle);
        std::fflush(stdout);
    });
}
