// drive_binned_absent.cpp — a build of the engine WITHOUT the launchers of binned_kernel.hip (no stand-in is linked: the weak references
// stay null) on the TEST-ONLY null device: fmhip_binned_cross_moments and fmhip_binned_evaluate answer FMHIP_ERR_UNSUPPORTED — after their
// argument checks, which still come first — and never fall back to the host definition; the host definition itself needs no launcher.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        fmhip_vec key = 0, x = 0, est = 0;
        OK(fmhip_vec_create_filled(1000, 1.0, &key));
        OK(fmhip_vec_create_filled(1000, 2.0, &x));
        const fmhip_vec xs[2] = { 0, x };
        const double bounds[1] = { 0.5 }, unsorted[2] = { 1.0, 0.0 }, coef[4] = { 1.0, 2.0, 3.0, 4.0 };
        int64_t counts[3]; double sums[16];
        EXPECT(fmhip_binned_cross_moments(key, unsorted, 3, xs, 2, &x, 1, counts, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_binned_cross_moments(key, bounds, 2, xs, 2, &x, 1, counts, sums), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_binned_evaluate(key, bounds, 2, xs, 2, coef, &est), FMHIP_ERR_UNSUPPORTED);
        if (est != 0) { std::fprintf(stderr, "a refused evaluation left a handle\n"); std::abort(); }
        const float k[3] = { 0.0f, 1.0f, 2.0f }; const float* none[1] = { nullptr };
        OK(fmhip_binned_cross_moments_host(k, 3, bounds, 2, none, 1, nullptr, 0, counts, sums));
        if (counts[0] != 1 || counts[1] != 2) { std::fprintf(stderr, "host definition: %lld %lld\n", (long long)counts[0], (long long)counts[1]); std::abort(); }
        OK(fmhip_vec_release(key)); OK(fmhip_vec_release(x));
        std::printf("cycle %d: binned absent done\n", cycle);
        std::fflush(stdout);
    });
}
