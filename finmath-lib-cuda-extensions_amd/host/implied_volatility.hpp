// implied_volatility.hpp — the definition of the IMPLIED VOLATILITY per path: the inverse of fm_option_formula's value in sigma, for the
// Black–Scholes and the Bachelier model, with the two partials a differentiation through a quoted volatility needs, in ONE header that the
// host (g++, hipcc -x c++) and the device (csrc/implied_volatility_kernel.hip) both compile.  DESIGN.md §4.25; contract: include/fmhip.h.
//
// The rules are normal_functions.hpp's: fp64, only + − × /, __builtin_sqrt, comparisons and integer operations, fm_exp64, fm_log64,
// fm_normal_density, fm_mills_ratio and fm_normal_quantile; every operation rounded once by IEEE 754 on either side (builds:
// -ffp-contract=off, no fast-math); no <cmath> transcendental, no OCML call.  What the device computes EQUALS what the host does.
//
//   fm_implied_volatility(model, price, F, N, root_T, K)   a CALL in forward form: price = N·(undiscounted value), root_T = √T.
//     c = price/N, intrinsic = max(F − K, 0), tv = c − intrinsic (in fp64), decided in THIS order:
//       a NaN among price, F, N, root_T, K; N <= 0 (or c a NaN)          NaN, NaN, NaN
//       c == intrinsic                                                   sigma +0, both partials NaN
//       root_T == 0; an infinite F or K; c < intrinsic                   NaN, NaN, NaN
//       Black–Scholes: F <= 0 or K <= 0; c > F                           NaN, NaN, NaN
//       Black–Scholes: c == F;  Bachelier: c == +∞                       sigma +∞, both partials NaN
//       live (Black–Scholes intrinsic < c < F, Bachelier intrinsic < c < ∞)
//                                                                        sigma the root; d_price = 1/(N·vega₁), d_forward = −delta₁/vega₁ with
//                                                                        vega₁, delta₁ = fm_option_formula(model, F, sigma, 1, root_T, K)'s
//     (every NaN here is the quiet NaN 0x7ff8000000000000, which fm_narrow turns into 0x7fc00000).
//
// THE SOLVER works with the time value on the out-of-the-money side and the total volatility s = σ√T.  Every iteration keeps a bracket
// [lo, hi] around the root: a Newton step that leaves it is replaced by the bracket's (geometric or arithmetic) middle, so no iterate
// is ever <= 0.  An iteration ends when a step is below 2⁻²⁸ of the iterate (Newton's error after that step is the square of it) — on the
// complement's side plus 2⁻⁴⁸, the size of the steps that the rounding of F − c alone causes, 2⁻⁴⁹·F in the price — or at
// FM_IMPLIED_MAX_ITERATIONS with the last iterate: no loop's exit depends on data alone.
//   Bachelier, m = |F − K|, u = m/s:  tv = s·φ(u) − m·Φ(−u).  m == 0: s = tv·√(2π).  q = tv/m >= 0.1 (u below 0.93): Newton on the value
//     itself in s (convex and increasing; the start is the root of the expansion to second order in u).  q < 0.1: Newton on
//     ln(tv/m) = −u²/2 − ln√(2π) + ln((1 − u·M(u))/u) in ln u, which is concave and decreasing: monotone from the start √(−2·ln(q·√(2π))),
//     which lies right of the root; the value itself is never formed, so the tail keeps its relative accuracy down to the last denormal.
//   Black–Scholes, A = min(F, K), B = max(F, K), L = ln(B/A), d₊ = s/2 − L/s, t₋ = s/2 + L/s; A·φ(d₊) = B·φ(t₋), so with Mills' ratio M
//     below the inflection point s_c = √(2L):   tv/A       = φ(d₊)·(M(−d₊) − M(t₋))     Newton on its logarithm in ln s, from the left
//     from s_c on:                              (F − c)/A  = φ(d₊)·(M(d₊) + M(t₋))      Newton on its logarithm in s
//     The complement to the upper bound is F − c, one subtraction of the inputs; it is never formed from two computed Φ's.  Which side
//     the root lies on is decided once, at s_c, where d₊ = 0.  Starts: the quantile of tv/A bounds the root from the left (tv/A < Φ(d₊));
//     −2·Φ⁻¹((F − c)/(A + B)) is the root itself at the money.  No exponential of d₊ is evaluated: φ(d₊) enters as −d₊²/2.
// Host only, below: implied_volatility_host (the definition over arrays) and its argument check, which complain with std::invalid_argument.
#pragma once
#include <stdint.h>

#include "normal_functions.hpp"

namespace fmhost {

enum { FM_IMPLIED_VOLATILITY = 1, FM_IMPLIED_D_PRICE = 2, FM_IMPLIED_D_FORWARD = 4, FM_IMPLIED_ALL = 7 };      // = FMHIP_IMPLIED_*
constexpr int FM_IMPLIED_MAX_OUTPUTS = 3;
constexpr int FM_IMPLIED_MAX_ITERATIONS = 64;                     // the bound of every iteration below
constexpr double FM_IMPLIED_STEP = 0x1p-28;                       // a relative step below this ends an iteration
constexpr double FM_LOG_SQRT_2PI = 0x1.d67f1c864beb5p-1;          // ln √(2π), rounded to nearest
constexpr double FM_SQRT_2PI = 0x1.40d931ff62706p+1;              // √(2π), rounded to nearest
constexpr double FM_IMPLIED_FLOOR = 0x1p-48;                      // … and, from the inflection point on, an absolute one: F − c carries 2⁻⁵³·F of rounding
constexpr double FM_IMPLIED_DIRECT_FROM = 0.1;                    // Bachelier: tv/m from which the value itself is iterated on
constexpr double FM_IMPLIED_MAX_TOTAL = 80.0;                     // Black–Scholes: 2·Φ(−s/2) is below the smallest denormal from here on

struct FmImpliedOut { double sigma, d_price, d_forward; };
struct FmImpliedRoot { double s; int iterations; bool converged; };      // s = σ√T; evaluations of the iterated function; the stopping rule met

// Bachelier: the s > 0 with s·φ(m/s) − m·Φ(−m/s) = tv, for tv > 0 and m >= 0 finite
FM_HD inline __attribute__((always_inline)) FmImpliedRoot fm_implied_total_bachelier(double tv, double m)
{
    FmImpliedRoot r; r.iterations = 0; r.converged = true;
    if (m == 0.0) { r.s = tv * FM_SQRT_2PI; return r; }
    double q = tv / m;
    if (!(q > 0.0)) q = fm_double(1ull);                                      // tv/m below the smallest denormal
    r.converged = false;
    if (q >= FM_IMPLIED_DIRECT_FROM) {
        // tv = s·φ₀ − m/2 + φ₀·m²/(2s) − …: the larger root of the quadratic
        const double a = tv + 0.5 * m, f0m = FM_INV_SQRT_2PI * m;
        double s = (a + __builtin_sqrt(a * a - 2.0 * (f0m * f0m))) / (2.0 * FM_INV_SQRT_2PI);
        if (!(s > 0.0)) s = a * FM_SQRT_2PI;
        double lo = 0.0, hi = fm_double(0x7ff0000000000000ull);
        for (int it = 1; it <= FM_IMPLIED_MAX_ITERATIONS; ++it) {
            r.iterations = it;
            const double u = m / s;
            const double density = fm_normal_density(u);
            const double residual = (s * density - tv) - m * (density * fm_mills_ratio(u));      // increasing in s
            if (residual < 0.0) lo = s; else hi = s;
            double next = s - residual / density;
            if (!(next >= lo && next <= hi) || !(next > 0.0)) next = hi - hi == 0.0 ? 0.5 * (lo + hi) : 2.0 * s;
            const double step = next - s;
            s = next;
            if ((step < 0.0 ? 0.0 - step : step) <= FM_IMPLIED_STEP * s) { r.converged = true; break; }
        }
        r.s = s;
        return r;
    }
    const double target = fm_log64(q) + FM_LOG_SQRT_2PI;                      // of −u²/2 + ln((1 − u·M(u))/u), which is below −u²/2 here
    double u = __builtin_sqrt(0.0 - 2.0 * target);
    double lo = 0.9, hi = u;                                                  // tv/m at u = 0.9 is 0.1088
    for (int it = 1; it <= FM_IMPLIED_MAX_ITERATIONS; ++it) {
        r.iterations = it;
        const double w = 1.0 - u * fm_mills_ratio(u);
        const double h = (fm_log64(w / u) - 0.5 * (u * u)) - target;          // decreasing in u
        if (h > 0.0) lo = u; else hi = u;
        double next = u * fm_exp64(h * w);                                    // d h / d ln u = −1/w
        if (!(next >= lo && next <= hi)) next = __builtin_sqrt(lo * hi);
        const double step = next - u;
        u = next;
        if ((step < 0.0 ? 0.0 - step : step) <= FM_IMPLIED_STEP * u) { r.converged = true; break; }
    }
    r.s = m / u;
    return r;
}

// Black–Scholes: the s > 0 with A·Φ(d₊) − B·Φ(d₋) = tv, given also complement = A − tv as the caller's ONE subtraction; 0 < A <= B finite,
// 0 < tv, 0 < complement
FM_HD inline __attribute__((always_inline)) FmImpliedRoot fm_implied_total_black_scholes(double tv, double complement, double A, double B)
{
    FmImpliedRoot r; r.iterations = 0; r.converged = false;
    const double ratio = B / A;
    const double L = fm_log64(ratio);
    const double s_c = __builtin_sqrt(2.0 * L);
    double beta = tv / A, gamma = complement / A;
    if (!(beta > 0.0)) beta = fm_double(1ull);
    if (!(gamma > 0.0)) gamma = fm_double(1ull);
    const double beta_c = FM_INV_SQRT_2PI * (fm_mills_ratio(0.0) - fm_mills_ratio(s_c));      // tv/A at s_c, where d₊ = 0
    if (beta < beta_c) {                                                       // below the inflection point (L > 0 here)
        const double target = fm_log64(beta) + FM_LOG_SQRT_2PI;               // of −d₊²/2 + ln(M(−d₊) − M(t₋))
        const double D = 0.0 - fm_normal_quantile(beta);                      // beta < Φ(d₊): d₊ > −D
        double s = 2.0 * L / (D + __builtin_sqrt(D * D + 2.0 * L));
        if (!(s > 0.0 && s <= s_c)) s = 0.5 * s_c;
        double lo = 0.5 * s, hi = s_c;
        for (int it = 1; it <= FM_IMPLIED_MAX_ITERATIONS; ++it) {
            r.iterations = it;
            const double x = L / s;
            double t_plus = x - 0.5 * s;
            if (!(t_plus > 0.0)) t_plus = 0.0;
            const double dM = fm_mills_ratio(t_plus) - fm_mills_ratio(x + 0.5 * s);
            const double h = (fm_log64(dM) - 0.5 * (t_plus * t_plus)) - target;      // increasing in s
            if (h < 0.0) lo = s; else hi = s;
            double next = s * fm_exp64(0.0 - h * dM / s);                     // d h / d ln s = s/dM
            if (!(next >= lo && next <= hi)) next = __builtin_sqrt(lo * hi);
            const double step = next - s;
            s = next;
            if ((step < 0.0 ? 0.0 - step : step) <= FM_IMPLIED_STEP * s) { r.converged = true; break; }
        }
        r.s = s;
        return r;
    }
    const double target = fm_log64(gamma) + FM_LOG_SQRT_2PI;                  // of −d₊²/2 + ln(M(d₊) + M(t₋))
    double s = 0.0 - 2.0 * fm_normal_quantile(gamma / (1.0 + ratio));
    if (!(s >= s_c)) s = s_c;
    if (!(s <= FM_IMPLIED_MAX_TOTAL)) s = FM_IMPLIED_MAX_TOTAL;
    if (!(s > 0.0)) s = fm_double(0x3cb0000000000000ull);                     // 2⁻⁵²: at the money with a complement that rounds to A
    double lo = s_c, hi = FM_IMPLIED_MAX_TOTAL;
    for (int it = 1; it <= FM_IMPLIED_MAX_ITERATIONS; ++it) {
        r.iterations = it;
        const double x = L / s;
        double d_plus = 0.5 * s - x;
        if (!(d_plus > 0.0)) d_plus = 0.0;
        const double S = fm_mills_ratio(d_plus) + fm_mills_ratio(0.5 * s + x);
        const double h = (fm_log64(S) - 0.5 * (d_plus * d_plus)) - target;    // decreasing in s
        if (h > 0.0) lo = s; else hi = s;
        double next = s + h * S;                                              // d h / d s = −1/S
        if (!(next >= lo && next <= hi) || !(next > 0.0)) next = lo > 0.0 ? 0.5 * (lo + hi) : 0.5 * s;
        const double step = next - s;
        s = next;
        if ((step < 0.0 ? 0.0 - step : step) <= FM_IMPLIED_STEP * s + FM_IMPLIED_FLOOR) { r.converged = true; break; }
    }
    r.s = s;
    return r;
}

// the classification of the header's comment and the solve; root_out (host tests) receives the iteration's record; without with_partials
// the partials are left NaN (a caller that asks for sigma alone: sigma is the same)
FM_HD inline __attribute__((always_inline)) FmImpliedOut fm_implied_volatility_counted(int model, double price, double F, double N, double root_T, double K, FmImpliedRoot* root_out, bool with_partials)
{
    const double nan = fm_double(0x7ff8000000000000ull), infinity = fm_double(0x7ff0000000000000ull);
    FmImpliedOut r;
    r.sigma = r.d_price = r.d_forward = nan;
    if (root_out) { root_out->s = nan; root_out->iterations = 0; root_out->converged = true; }
    if (price != price || F != F || N != N || root_T != root_T || K != K || !(N > 0.0)) return r;
    const double c = price / N;
    if (c != c) return r;
    const double intrinsic = F - K > 0.0 ? F - K : 0.0;
    if (c == intrinsic) { r.sigma = 0.0; return r; }
    if (!(root_T > 0.0) || F - F != 0.0 || K - K != 0.0 || c < intrinsic) return r;
    const double tv = c - intrinsic;
    FmImpliedRoot root;
    if (model == FM_FORMULA_BLACK_SCHOLES) {
        if (!(F > 0.0) || !(K > 0.0) || c > F) return r;
        if (c == F) { r.sigma = infinity; return r; }
        root = fm_implied_total_black_scholes(tv, F - c, F < K ? F : K, F < K ? K : F);
    } else {
        if (c == infinity) { r.sigma = infinity; return r; }
        const double m = F - K;
        root = fm_implied_total_bachelier(tv, m < 0.0 ? 0.0 - m : m);
    }
    if (root_out) *root_out = root;
    r.sigma = root.s / root_T;
    if (!with_partials || r.sigma == 0.0 || r.sigma == infinity) return r;    // (a root that under- or overflows in the division)
    const FmFormulaOut at = fm_option_formula(model, F, r.sigma, 1.0, root_T, K);
    r.d_price = 1.0 / (N * at.vega);
    r.d_forward = (0.0 - at.delta) / at.vega;
    return r;
}
FM_HD inline __attribute__((always_inline)) FmImpliedOut fm_implied_volatility(int model, double price, double F, double N, double root_T, double K)
{
    return fm_implied_volatility_counted(model, price, F, N, root_T, K, nullptr, true);
}
FM_HD inline __attribute__((always_inline)) FmImpliedOut fm_implied_volatility_masked(int model, double price, double F, double N, double root_T, double K, bool with_partials)
{
    return fm_implied_volatility_counted(model, price, F, N, root_T, K, nullptr, with_partials);
}

} // namespace fmhost

// ---------------------------------------------------------------- host only: the argument check and the definition over arrays
#if !defined(__HIP_DEVICE_COMPILE__)
namespace fmhost {

// what can be said about fmhip_implied_volatility's arguments without looking at a vector
inline void impliedCheck(int model, double maturity, double strike, int outputs, const void* out)
{
    if (model < 0 || model >= FM_FORMULA_MODELS) throw std::invalid_argument("implied volatility: unknown model " + std::to_string(model));
    if (!(maturity >= 0.0) || maturity - maturity != 0.0) throw std::invalid_argument("implied volatility: the maturity is finite and not negative");
    if (strike - strike != 0.0) throw std::invalid_argument("implied volatility: the strike is finite");
    if (outputs < 1 || outputs > FM_IMPLIED_ALL) throw std::invalid_argument("implied volatility: outputs is a mask of volatility (1), d/d price (2) and d/d forward (4)");
    if (!out) throw std::invalid_argument("implied volatility: null pointer: out");
}

// price, forward, payoff_unit: an array of n floats, or NULL for the scalar beside it; out: one array per set bit of outputs, in bit order
inline void implied_volatility_host(int model, const float* price, double price_scalar, const float* forward, double forward_scalar,
                                    const float* payoff_unit, double payoff_unit_scalar, int64_t n, double maturity, double strike, int outputs, float* const* out)
{
    impliedCheck(model, maturity, strike, outputs, out);
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("implied volatility: of " + std::to_string(n) + " elements (1 … 2^31)");
    const int n_out = fm_formula_outputs(outputs);
    for (int f = 0; f < n_out; ++f) if (!out[f]) throw std::invalid_argument("implied volatility: null pointer: out[" + std::to_string(f) + "]");
    const double root_T = __builtin_sqrt(maturity);
    for (int64_t p = 0; p < n; ++p) {
        const FmImpliedOut r = fm_implied_volatility(model, price ? (double)price[p] : price_scalar, forward ? (double)forward[p] : forward_scalar,
                                                     payoff_unit ? (double)payoff_unit[p] : payoff_unit_scalar, root_T, strike);
        int f = 0;
        if (outputs & FM_IMPLIED_VOLATILITY) out[f++][p] = fm_narrow(r.sigma);
        if (outputs & FM_IMPLIED_D_PRICE) out[f++][p] = fm_narrow(r.d_price);
        if (outputs & FM_IMPLIED_D_FORWARD) out[f++][p] = fm_narrow(r.d_forward);
    }
}

} // namespace fmhost
#endif
