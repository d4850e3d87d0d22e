// gamma_icdf.hpp — the definition of the gamma and the exponential law of host/increments.hpp, in ONE header that the host (g++, hipcc -x c++)
// and the device (mt_bm_kernel.hip: MtLevyDraw) both compile.  DESIGN.md §4.11.
//
// A normal tail draw goes through log, which two math libraries round differently by an ulp now and then (§4.9's one-ulp clause).  These
// laws need exp and log inside an iteration, so their definition is written here with + − × /, sqrt, comparisons and integer operations on
// the bits of a double only — every one of them rounded once, by IEEE 754, on either side (builds: -ffp-contract=off, no fast-math) — and
// the draws of the device EQUAL the host's by construction, as the Poisson draws do.  No <cmath> transcendental, no OCML call.
//
//   fm_exp64, fm_log64         argument reduction on the exponent bits, the two-constant split of ln 2 (Cody–Waite), the polynomials of
//                              fdlibm's e_exp.c / e_log.c in Horner form; below one ulp of error on paper, NOT correctly rounded — they
//                              need to be the same on both sides, and they are
//   fm_gamma_p                 regularised lower incomplete gamma function P(shape, x): the power series for x < shape + 1, the continued
//                              fraction for Q = 1 − P by the modified Lentz method otherwise (Press et al., Numerical Recipes §6.2); each
//                              ends when another term no longer changes the value, and after a fixed number of terms at the latest
//   fm_inverse_gamma_cdf       min-free root of P(shape, x) = u: a guess — (u·Γ(shape + 1))^(1/shape), the small-x form, or Wilson–Hilferty
//                              through AS 241 — then Halley steps (NR §6.2.1) on P − u below x = shape + 1 and on (1 − u) − Q above it,
//                              where 1 − u is exact, so that the upper tail keeps its relative accuracy; ends when a step is below 2^-30
//                              of the iterate, and after FM_GAMMA_HALLEY_CAP steps at the latest
//   fm_exponential_icdf        −log(1 − u) / rate
// What depends on the shape alone (FmGammaConsts: lgamma(shape) among it) is computed by the HOST, once per distinct shape, and only read
// here: host/increments.hpp builds it and hands it to the device in IncrementLaws::tables.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define FM_HD __host__ __device__
#else
#define FM_HD
#endif

namespace fmhost {

// The supported shapes; everything outside is refused by checkedIncrementLaws (tests/test_gamma_icdf_cpu.py holds the accuracy inside).
constexpr double FM_GAMMA_SHAPE_MIN = 0.01, FM_GAMMA_SHAPE_MAX = 1000.0;
constexpr int FM_GAMMA_SERIES_CAP = 4000;          // terms of the power series (shape 1000 at x = 1001 needs some 330)
constexpr int FM_GAMMA_FRACTION_CAP = 4000;        // levels of the continued fraction (shape 1000 at x = 1001 needs some 300)
constexpr int FM_GAMMA_HALLEY_CAP = 40;            // steps of the iteration (the test grid needs at most 12)

// Per distinct shape, from the host: indices into the law's entry of IncrementLaws::tables
enum { FM_GC_LGAMMA = 0,       // lgamma(shape)
       FM_GC_INV_SHAPE,        // 1 / shape
       FM_GC_LGAMMA1,          // lgamma(shape + 1)
       FM_GC_WH_CENTRE,        // 1 − 1/(9·shape)                  Wilson–Hilferty: x = shape · (centre + z · slope)^3
       FM_GC_WH_SLOPE,         // 1 / (3·sqrt(shape))
       FM_GC_SPLIT,            // shape <= 1: below this u the guess is the small-x form, above it 1 − log((1 − u)/(1 − split))
       FM_GAMMA_CONSTS };

FM_HD inline uint64_t fm_bits(double d) { uint64_t b; __builtin_memcpy(&b, &d, 8); return b; }
FM_HD inline double fm_double(uint64_t b) { double d; __builtin_memcpy(&d, &b, 8); return d; }

// e^x.  x = k·ln 2 + r, |r| <= ln 2 / 2; e^r by fdlibm's rational form of a degree-5 polynomial in r²; 2^k in two exact-or-final factors.
FM_HD inline double fm_exp64(double x)
{
    if (x != x) return x;
    if (x > 709.782712893384) return fm_double(0x7ff0000000000000ull);
    if (x < -745.2) return 0.0;
    const double kf = x * 1.44269504088896338700e+00;
    const int k = (int)(kf < 0.0 ? kf - 0.5 : kf + 0.5);
    const double hi = x - (double)k * 6.93147180369123816490e-01;         // exact: the constant has 32 trailing zero bits
    const double lo = (double)k * 1.90821492927058770002e-10;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (1.66666666666666019037e-01 + t * (-2.77777777770155933842e-03 + t * (6.61375632143793436117e-05
                         + t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    const int k1 = k / 2, k2 = k - k1;                                      // both within the normal exponents; the second product rounds, once
    return y * fm_double((uint64_t)(k1 + 1023) << 52) * fm_double((uint64_t)(k2 + 1023) << 52);
}

// ln x.  x = 2^k · m, sqrt(2)/2 <= m < sqrt(2); f = m − 1, s = f/(2 + f); fdlibm's degree-7 polynomial in s².
FM_HD inline double fm_log64(double x)
{
    if (x != x || x < 0.0) return fm_double(0x7ff8000000000000ull);
    if (x == 0.0) return fm_double(0xfff0000000000000ull);
    uint64_t b = fm_bits(x);
    if (b >= 0x7ff0000000000000ull) return x;
    int k = 0;
    if (b < 0x0010000000000000ull) { b = fm_bits(x * 0x1.0p54); k = -54; }   // a subnormal: exact scaling
    k += (int)(b >> 52) - 1023;
    uint64_t m = b & 0x000fffffffffffffull;
    if (m >= 0x6a09e667f3bcdull) k += 1;                                      // mantissa of sqrt(2): m/2 takes the exponent up
    const double f = fm_double(m | (m >= 0x6a09e667f3bcdull ? 0x3fe0000000000000ull : 0x3ff0000000000000ull)) - 1.0;
    const double dk = (double)k;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

// Wichura's AS 241 (PPND16) with fm_log64 in the tails: host/mersenne.hpp's inverseNormalCdf but for that one call.  Only the guess uses it.
FM_HD inline double fm_normal_quantile(double p)
{
    const double q = p - 0.5;
    if (__builtin_fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r
                        + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e0)
                 / (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r
                        + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
    }
    double r = __builtin_sqrt(0.0 - fm_log64(q < 0 ? p : 1.0 - p));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        val = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e0) * r
                   + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r + 4.63033784615654529590e0) * r + 1.42343711074968357734e0)
            / (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r
                   + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r + 2.05319162663775882187e0) * r + 1.0);
    } else {
        r -= 5.0;
        val = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r
                   + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r + 5.46378491116411436990e0) * r + 6.65790464350110377720e0)
            / (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r
                   + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
    }
    return q < 0.0 ? -val : val;
}

// For x > 0: P(shape, x) below x = shape + 1, by the series, and Q = 1 − P from there on, by the continued fraction — whichever is computed
// directly, and so keeps its relative accuracy — and front = x^shape e^−x / Γ(shape), x times the density.
struct FmGammaTail { double direct, front; };
FM_HD inline __attribute__((always_inline)) FmGammaTail fm_gamma_tail(double shape, double lgamma_shape, double x)
{
    FmGammaTail r;
    r.front = fm_exp64(shape * fm_log64(x) - x - lgamma_shape);
    if (x < shape + 1.0) {
        double denominator = shape, term = 1.0, sum = 1.0;
        for (int n = 0; n < FM_GAMMA_SERIES_CAP; ++n) {
            denominator += 1.0;
            term = term * x / denominator;
            const double before = sum;
            sum += term;
            if (sum == before) break;
        }
        r.direct = r.front * sum / shape;
    } else {
        const double tiny = 0x1.0p-1000;
        double b = x + 1.0 - shape, c = 0x1.0p1000, d = 1.0 / b, h = d;
        for (int i = 1; i <= FM_GAMMA_FRACTION_CAP; ++i) {
            const double an = (0.0 - (double)i) * ((double)i - shape);
            b += 2.0;
            d = an * d + b;
            if (__builtin_fabs(d) < tiny) d = tiny;
            c = b + an / c;
            if (__builtin_fabs(c) < tiny) c = tiny;
            d = 1.0 / d;
            const double del = d * c;
            h *= del;
            if (__builtin_fabs(del - 1.0) <= 0x1.0p-52) break;
        }
        r.direct = r.front * h;
    }
    return r;
}

FM_HD inline double fm_gamma_p(double shape, double lgamma_shape, double x)
{
    if (!(x > 0.0)) return 0.0;
    const double direct = fm_gamma_tail(shape, lgamma_shape, x).direct;
    return x < shape + 1.0 ? direct : 1.0 - direct;
}

// x with P(shape, x) = u, 0 <= u < 1; consts: the shape's FM_GAMMA_CONSTS doubles.  u = 0 → +0.0.
FM_HD inline double fm_inverse_gamma_cdf(double shape, const double* consts, double u)
{
    if (!(u > 0.0)) return 0.0;
    const double q = 1.0 - u;                                               // exact: u is a multiple of 2^-53 (2^-52 from nextDouble)
    const double lgamma_shape = consts[FM_GC_LGAMMA];
    // the small-x form: P(x) <= x^shape / Γ(shape + 1), so this is never above the root
    double x = fm_exp64((fm_log64(u) + consts[FM_GC_LGAMMA1]) * consts[FM_GC_INV_SHAPE]);
    if (shape > 1.0) {
        const double w = consts[FM_GC_WH_CENTRE] + fm_normal_quantile(u) * consts[FM_GC_WH_SLOPE];
        const double wilson_hilferty = shape * (w * w * w);
        if (w > 0.0 && wilson_hilferty > x) x = wilson_hilferty;
    } else if (u >= consts[FM_GC_SPLIT]) {
        x = 1.0 - fm_log64(q / (1.0 - consts[FM_GC_SPLIT]));
    }
    if (!(x > 0.0)) return 0.0;                                             // the root lies below the smallest double
    for (int step = 0; step < FM_GAMMA_HALLEY_CAP; ++step) {
        const FmGammaTail tail = fm_gamma_tail(shape, lgamma_shape, x);
        const double error = x < shape + 1.0 ? tail.direct - u : q - tail.direct;
        const double density = tail.front / x;
        if (!(density > 0.0) || !(density < 0x1.0p1023)) break;           // nothing to divide by: x is as good as it gets
        const double newton = error / density;
        double curvature = newton * ((shape - 1.0) / x - 1.0);            // Halley: f''/f' = (shape − 1)/x − 1
        if (curvature > 1.0) curvature = 1.0;
        const double move = newton / (1.0 - 0.5 * curvature);
        double next = x - move;
        if (!(next > 0.0)) next = 0.5 * x;
        const bool settled = __builtin_fabs(move) <= 0x1.0p-30 * next;
        x = next;
        if (settled) break;
    }
    return x;
}

// −log(1 − u) / rate; 1 − u is exact; u = 0 → +0.0 (0 − (+0) = +0)
FM_HD inline double fm_exponential_icdf(double rate, double u)
{
    return (0.0 - fm_log64(1.0 - u)) / rate;
}

} // namespace fmhost
