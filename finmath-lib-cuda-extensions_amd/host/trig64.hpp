// trig64.hpp — the SINE and COSINE of a double, as a pair, in ONE header that the host (g++, hipcc -x c++) and the device
// (csrc/transform_kernel.hip) both compile.  DESIGN.md §4.28.
//
// The rules are gamma_icdf.hpp's: fp64, only + − × /, comparisons and integer operations; every operation rounded once by IEEE 754 on
// either side (builds: -ffp-contract=off, no fast-math); no <cmath>, no OCML call.  What the device computes EQUALS what the host does.
//
//   fm_sincos64(θ)   n = round(θ·2/π) (half away from zero), r = (θ − n·P1) − n·P2 with π/2 = P1 + P2 + … (trig_coefficients.hpp, written by
//                    tools/trig_coefficients.py with mpmath): P1 has 33 bits, so n·P1 is exact for |n| < 2^20, and θ − n·P1 is exact as well
//                    (both are multiples of the smaller of their last places, and the difference is below π/4 + 2^-16 in size); n·P2 and the
//                    second subtraction round, by less than 2^-54 together; what π/2 has beyond P2 is below 2^-86, times n below 2^-66.
//                    Then sin r = r + (r·t)·S(t), cos r = (1 − t/2) + (t·t)·C(t), t = r·r, and the quadrant n mod 4 picks and signs them.
//   THE CONTRACT is an ABSOLUTE error:  |sin − sin θ| <= FM_TRIG_ERROR_ULPS·2⁻⁵³ and the same for the cosine, for |θ| <= FM_TRIG_MAX = 2^20.
//                    No relative accuracy is claimed near the zeros: the users here sum exp·cos terms and need none.  The constant is four
//                    times the one measured against mpmath (tests/test_transform_formula_cpu.py).
//                    |θ| > FM_TRIG_MAX, ±∞ and NaN give (NaN, NaN).  The sine is odd and the cosine even, bit for bit: every step is
//                    symmetric in the sign, and a sign is changed on the bits, so that a zero keeps its own.
#pragma once
#include <stdint.h>

#include "gamma_icdf.hpp"
#include "trig_coefficients.hpp"

namespace fmhost {

constexpr double FM_TRIG_ERROR_ULPS = 6.25;           // 4 × the measured 1.54 (sine) / 1.52 (cosine), rounded up

struct FmSinCos { double sin, cos; };

FM_HD inline double fm_flip_sign(double x) { return fm_double(fm_bits(x) ^ 0x8000000000000000ull); }

FM_HD inline FmSinCos fm_sincos64(double theta)
{
    FmSinCos out;
    if (!(theta >= 0.0 - FM_TRIG_MAX && theta <= FM_TRIG_MAX)) {
        out.sin = out.cos = fm_double(0x7ff8000000000000ull);
        return out;
    }
    const double kf = theta * FM_TRIG_2_OVER_PI;
    const int n = (int)(kf < 0.0 ? kf - 0.5 : kf + 0.5);
    const double fn = (double)n;
    const double r = (theta - fn * FM_TRIG_PIO2_1) - fn * FM_TRIG_PIO2_2;
    const double t = r * r;
    double S = FM_TRIG_SIN_COEFFICIENTS[FM_TRIG_SIN_DEGREE];
    for (int j = FM_TRIG_SIN_DEGREE - 1; j >= 0; --j) S = S * t + FM_TRIG_SIN_COEFFICIENTS[j];
    double C = FM_TRIG_COS_COEFFICIENTS[FM_TRIG_COS_DEGREE];
    for (int j = FM_TRIG_COS_DEGREE - 1; j >= 0; --j) C = C * t + FM_TRIG_COS_COEFFICIENTS[j];
    const double s = r == 0.0 ? r : r + (r * t) * S;                            // (−0 + +0 would lose the sign of a zero)
    const double c = (1.0 - 0.5 * t) + (t * t) * C;
    const bool swap = (n & 1) != 0;
    const double s_mag = swap ? c : s, c_mag = swap ? s : c;
    out.sin = (n & 2) != 0 ? fm_flip_sign(s_mag) : s_mag;                       // quadrants 2 and 3
    out.cos = ((n + 1) & 2) != 0 ? fm_flip_sign(c_mag) : c_mag;                 // quadrants 1 and 2
    return out;
}
FM_HD inline double fm_sin64(double theta) { return fm_sincos64(theta).sin; }
FM_HD inline double fm_cos64(double theta) { return fm_sincos64(theta).cos; }

} // namespace fmhost
