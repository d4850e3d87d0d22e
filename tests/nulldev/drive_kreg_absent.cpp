// drive_kreg_absent.cpp — a build of the engine WITHOUT the launcher of kreg_kernel.hip (no stand-in for it is linked: the weak reference
// stays null) on the TEST-ONLY null device: fmhip_kernel_moments answers FMHIP_ERR_UNSUPPORTED — after its argument checks, which still come
// first — and never falls back; the host-only call (fmhip_kernel_moments_host) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> k((size_t)n), y((size_t)n);
        for (int64_t p = 0; p < n; ++p) { k[(size_t)p] = (float)((p * 37) % 101) * 0.125f; y[(size_t)p] = (float)((int)((p * 5) % 17) - 8); }
        fmhip_vec hk = 0, hy = 0;
        OK(fmhip_vec_create_from_float(k.data(), n, &hk));
        OK(fmhip_vec_create_from_float(y.data(), n, &hy));
        const double points[3] = { 2.0, 6.0, 10.0 }, h[3] = { 2.0, 2.0, 2.0 }, close[3] = { 2.0, 3.0, 4.0 }, shrinking[3] = { 2.0, 0.5, 2.0 };      // close ± shrinking: lower 0, 2.5, 2
        double sums[3 * 5], want[3 * 5];
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_kernel_moments(hk, close, shrinking, 3, FMHIP_KERNEL_UNIFORM, 0, &hy, 1, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_kernel_moments(hk, points, h, 3, FMHIP_KERNEL_UNIFORM, 2, &hy, 1, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_kernel_moments(hk, points, h, 3, FMHIP_KERNEL_UNIFORM, 0, &hy, 1, sums), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_kernel_moments(hk, points, h, 3, FMHIP_KERNEL_TRIWEIGHT, 1, &hy, 1, sums), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_kernel_moments(hk, points, h, 3, FMHIP_KERNEL_EPANECHNIKOV, 0, nullptr, 0, sums), FMHIP_ERR_UNSUPPORTED);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        const float* py[1] = { y.data() };
        OK(fmhip_kernel_moments_host(k.data(), n, points, h, 3, FMHIP_KERNEL_UNIFORM, 1, py, 1, sums));
        for (int q = 0; q < 3; ++q) {                                          // dyadic data: every sum is exact
            double w = 0, wd = 0, wdd = 0, wy = 0, wdy = 0;
            for (int64_t p = 0; p < n; ++p) {
                const double x = (double)k[(size_t)p], d = x - points[q];
                if (!(points[q] - 2.0 < x && x < points[q] + 2.0)) continue;
                w += 1.0; wd += d; wdd += d * d; wy += (double)y[(size_t)p]; wdy += d * (double)y[(size_t)p];
            }
            want[q * 5] = w; want[q * 5 + 1] = wd; want[q * 5 + 2] = wdd; want[q * 5 + 3] = wy; want[q * 5 + 4] = wdy;
        }
        if (std::memcmp(sums, want, sizeof sums) != 0) { std::fprintf(stderr, "the definition is off\n"); std::abort(); }
        OK(fmhip_vec_release(hk)); OK(fmhip_vec_release(hy));
        std::printf("cycle %d: kreg absent done\n", cycle);
        std::fflush(stdout);
    });
}
