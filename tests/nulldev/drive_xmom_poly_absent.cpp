// drive_xmom_poly_absent.cpp — a build of the engine WITHOUT the launchers of xmom_poly_kernel.hip (no stand-in is linked: the weak references
// stay null) on the TEST-ONLY null device: fmhip_polynomial_cross_moments and fmhip_polynomial_evaluate answer FMHIP_ERR_UNSUPPORTED — after
// their argument checks, which still come first — and never fall back.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        fmhip_vec a = 0, b = 0, out = 0;
        OK(fmhip_vec_create_filled(1000, 1.0, &a));
        OK(fmhip_vec_create_filled(999, 2.0, &b));
        const fmhip_vec states[2] = { a, a }, bad[2] = { a, b };
        const uint8_t e[6] = { 0, 0, 1, 0, 1, 2 }, seven[2] = { 7, 0 };
        const double c[3] = { 1.0, 2.0, 3.0 };
        double sums[16];
        EXPECT(fmhip_polynomial_cross_moments(states, 2, seven, 1, nullptr, 0, &a, 1, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_polynomial_cross_moments(bad, 2, e, 3, nullptr, 0, &a, 1, sums), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_polynomial_cross_moments(states, 2, e, 3, nullptr, 0, &a, 1, sums), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_polynomial_evaluate(states, 0, e, 3, nullptr, 0, c, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_polynomial_evaluate(bad, 2, e, 3, nullptr, 0, c, &out), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_polynomial_evaluate(states, 2, e, 3, nullptr, 0, c, &out), FMHIP_ERR_UNSUPPORTED);
        OK(fmhip_vec_release(a)); OK(fmhip_vec_release(b));
        std::printf("cycle %d: xmom poly absent done\n", cycle);
        std::fflush(stdout);
    });
}
