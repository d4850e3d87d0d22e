// drive_table_absent.cpp — a build of the engine WITHOUT the launcher of table_kernel.hip (no stand-in for it is linked: the weak reference
// stays null) on the TEST-ONLY null device: fmhip_table_apply answers FMHIP_ERR_UNSUPPORTED — after its argument checks, which still come
// first — and never falls back; the host-only calls (fmhip_table_build, fmhip_table_apply_host) need no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101) * 0.125f;
        fmhip_vec v = 0, out[2] = { 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        const double knots[4] = { 0.0, 4.0, 8.0, 12.0 }, values[4] = { 1.0, 3.0, 2.0, 5.0 }, unsorted[4] = { 0.0, 4.0, 4.0, 12.0 };
        double coef[2 * 5 * 4];
        OK(fmhip_table_build(knots, values, 4, FMHIP_TABLE_LINEAR, FMHIP_TABLE_CONSTANT, 0, coef));
        OK(fmhip_table_build(knots, values, 4, FMHIP_TABLE_LINEAR, FMHIP_TABLE_CONSTANT, 1, coef + 20));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_table_apply(v, unsorted, 4, coef, 2, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_table_apply(v, knots, 4, coef, 5, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_table_apply(v, knots, 4, coef, 1, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_table_apply(v, knots, 4, coef, 2, out), FMHIP_ERR_UNSUPPORTED);
        if (out[0] != 0 || out[1] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> value((size_t)n, -1.0f), slope((size_t)n, -1.0f);
        float* cols[2] = { value.data(), slope.data() };
        OK(fmhip_table_apply_host(a.data(), n, knots, 4, coef, 2, cols));
        for (int64_t p = 0; p < n; ++p) {                                       // dyadic data: the linear interpolant is exact
            const double X = (double)a[(size_t)p];
            const int s = X < 4.0 ? 0 : X < 8.0 ? 1 : 2;
            const double want = X >= 12.0 ? 5.0 : values[s] + (values[s + 1] - values[s]) / 4.0 * (X - knots[s]);
            const double want_slope = X >= 12.0 ? 0.0 : (values[s + 1] - values[s]) / 4.0;
            if ((double)value[(size_t)p] != want || (double)slope[(size_t)p] != want_slope) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)p); std::abort(); }
        }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: table absent done\n", cycle);
        std::fflush(stdout);
    });
}
