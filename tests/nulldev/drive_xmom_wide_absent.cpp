// drive_xmom_wide_absent.cpp — a build of the engine WITHOUT the launcher of xmom_wide_kernel.hip (no stand-in is linked: the weak reference
// stays null) on the TEST-ONLY null device: fmhip_cross_moments_wide answers FMHIP_ERR_UNSUPPORTED — after its argument checks, which still
// come first — and never falls back.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        fmhip_vec a = 0, b = 0;
        OK(fmhip_vec_create_filled(1000, 1.0, &a));
        OK(fmhip_vec_create_filled(999, 2.0, &b));
        const fmhip_vec xs[3] = { 0, a, a }, bad[2] = { a, b };
        double sums[16];
        EXPECT(fmhip_cross_moments_wide(xs, 0, nullptr, 0, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_cross_moments_wide(bad, 2, nullptr, 0, sums), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_cross_moments_wide(xs, 3, &a, 1, sums), FMHIP_ERR_UNSUPPORTED);
        OK(fmhip_vec_release(a)); OK(fmhip_vec_release(b));
        std::printf("cycle %d: xmom wide absent done\n", cycle);
        std::fflush(stdout);
    });
}
