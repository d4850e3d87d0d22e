// normal_functions.hpp — the definition of the NAMED FUNCTIONS of a vector's elements (the normal distribution function Φ, its density φ,
// its quantile Φ⁻¹) and of the closed-form OPTION FORMULAS per path (Black–Scholes and Bachelier: value, delta, vega of a call in forward
// form), in ONE header that the host (g++, hipcc -x c++) and the device (csrc/analytic_kernel.hip) both compile.  DESIGN.md §4.21;
// contract: include/fmhip.h.
//
// The rules are gamma_icdf.hpp's: fp64, only + − × /, __builtin_sqrt, comparisons and integer operations, fm_exp64 and fm_log64; every
// operation rounded once by IEEE 754 on either side (builds: -ffp-contract=off, no fast-math); no <cmath> transcendental, no OCML call.
// What the device computes EQUALS what the host does, by construction.
//
//   fm_normal_density(X)       φ(X) = fm_exp64(−X·X/2) · (1/√(2π)).  For X = (double) of an fp32 number X·X is exact (48 bits), and the error
//                              is fm_exp64's alone; for any other double the square's rounding adds |X|²·2⁻⁵⁴ relative.  φ(±∞) = 0.
//   fm_normal_cdf(X)           Φ(X).  For X <= 0: φ(X) · M(−X) with the Mills ratio M(t) = Φ(−t)/φ(t), a smooth function fitted piecewise
//                              (normal_cdf_coefficients.hpp, written by tools/normal_cdf_coefficients.py with mpmath: six pieces of t below 8
//                              as polynomials in t − centre, and (1/t) · P(1/t² − centre) from 8 on): a product of two factors that each
//                              have relative accuracy, so Φ keeps it down to the smallest denormal.  For X > 0: 1 − Φ(−X).  Φ(−∞) = 0,
//                              Φ(+∞) = 1.  Nothing here assumes that X is an fp32 number.
//   fm_normal_quantile_checked(U)   fm_normal_quantile (gamma_icdf.hpp: AS 241) with its ends: U = 0 → −∞, U = 1 → +∞, U < 0, U > 1 or a NaN → NaN.
//   fm_function_value(kind, x) the three as functions of an fp32 element: X = (double)x, the result narrowed once; a NaN result is the
//                              quiet NaN 0x7fc00000 (the table pass's).
//   fm_option_formula(...)     see FmFormulaOut below.
// Host only, below: function_apply_host and option_formula_host (the definitions over arrays) and their argument checks, which complain
// with std::invalid_argument.
#pragma once
#include <stdint.h>

#include "gamma_icdf.hpp"
#include "normal_cdf_coefficients.hpp"

namespace fmhost {

enum { FM_FN_NORMAL_CDF = 0, FM_FN_NORMAL_DENSITY = 1, FM_FN_NORMAL_QUANTILE = 2, FM_FN_KINDS = 3 };      // = FMHIP_FN_*
enum { FM_FORMULA_BLACK_SCHOLES = 0, FM_FORMULA_BACHELIER = 1, FM_FORMULA_MODELS = 2 };                   // = FMHIP_FORMULA_*
enum { FM_FORMULA_VALUE = 1, FM_FORMULA_DELTA = 2, FM_FORMULA_VEGA = 4, FM_FORMULA_ALL = 7 };
constexpr int FM_FN_MAX_FUNCTIONS = 4;
constexpr int FM_FORMULA_MAX_OUTPUTS = 3;
FM_HD inline int fm_formula_outputs(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }      // new vectors of a mask

FM_HD inline float fm_canonical_nan() { const uint32_t b = 0x7fc00000u; float f; __builtin_memcpy(&f, &b, 4); return f; }
FM_HD inline float fm_narrow(double r) { return r != r ? fm_canonical_nan() : (float)r; }

FM_HD inline double fm_normal_density(double X)
{
    return fm_exp64(0.0 - (X * X) * 0.5) * FM_INV_SQRT_2PI;
}

// M(t) for t >= 0 (a NaN comes back as a NaN; t = +∞ gives +0)
FM_HD inline double fm_mills_ratio(double t)
{
    int k = 0;
    for (int i = 0; i < FM_MILLS_PIECES - 1; ++i) k += t >= FM_MILLS_BREAKS[i] ? 1 : 0;
    double v = t, front = 1.0;
    if (t >= FM_MILLS_TAIL) { front = 1.0 / t; v = front * front; }          // the rare side: one division more
    const double s = v - FM_MILLS_CENTRES[k];
    const double* c = FM_MILLS_COEFFICIENTS[k];
    double p = c[FM_MILLS_DEGREE];
    for (int j = FM_MILLS_DEGREE - 1; j >= 0; --j) p = p * s + c[j];
    return front * p;
}

// Φ(X) from density = fm_normal_density(X), for a caller that wants both (φ is even, and so is its computation: X·X)
FM_HD inline double fm_normal_cdf_with(double X, double density)
{
    const double t = X < 0.0 ? 0.0 - X : X;
    const double lower = density * fm_mills_ratio(t);                           // Φ(−|X|); a NaN stays one
    return X > 0.0 ? 1.0 - lower : lower;
}
FM_HD inline double fm_normal_cdf(double X) { return fm_normal_cdf_with(X, fm_normal_density(X)); }

FM_HD inline double fm_normal_quantile_checked(double U)
{
    if (!(U >= 0.0) || !(U <= 1.0)) return fm_double(0x7ff8000000000000ull);
    if (U == 0.0) return fm_double(0xfff0000000000000ull);
    if (U == 1.0) return fm_double(0x7ff0000000000000ull);
    return fm_normal_quantile(U);
}

FM_HD inline float fm_function_value(int kind, float x)
{
    const double X = (double)x;
    return fm_narrow(kind == FM_FN_NORMAL_CDF ? fm_normal_cdf(X) : kind == FM_FN_NORMAL_DENSITY ? fm_normal_density(X) : fm_normal_quantile_checked(X));
}

// A call in forward form: forward F, volatility σ, payoff unit N (a discount factor, a notional, an annuity), maturity T >= 0, strike K;
// root_T = __builtin_sqrt(T), computed by the caller once; s = σ·root_T.
//   Black–Scholes:  d₊ = (fm_log64(F/K) + ½s²)/s, d₋ = d₊ − s;  value N·(F·Φ(d₊) − K·Φ(d₋)), delta N·Φ(d₊), vega N·F·φ(d₊)·√T
//   Bachelier:      d = (F − K)/s;                              value N·((F − K)·Φ(d) + s·φ(d)), delta N·Φ(d), vega N·√T·φ(d)
// Degenerate — not s > 0, and for Black–Scholes also not F > 0 or not K > 0 —: the limit, value N·max(F − K, 0), delta N·[F > K], vega 0.
// A NaN among F, σ, N, K, root_T: a NaN in every output.  Every operation in fp64, rounded on its own; narrowed by the caller (fm_narrow).
struct FmFormulaOut { double value, delta, vega; };
FM_HD inline FmFormulaOut fm_option_formula(int model, double F, double sigma, double N, double root_T, double K)
{
    FmFormulaOut r;
    if (F != F || sigma != sigma || N != N || K != K || root_T != root_T) {
        r.value = r.delta = r.vega = fm_double(0x7ff8000000000000ull);
        return r;
    }
    const double s = sigma * root_T;
    const bool live = s > 0.0 && (model != FM_FORMULA_BLACK_SCHOLES || (F > 0.0 && K > 0.0));
    if (!live) {                                                               // the rare side
        const double intrinsic = F - K;
        r.value = N * (intrinsic > 0.0 ? intrinsic : 0.0);
        r.delta = N * (F > K ? 1.0 : 0.0);
        r.vega = 0.0;
        return r;
    }
    if (model == FM_FORMULA_BLACK_SCHOLES) {
        const double d_plus = (fm_log64(F / K) + 0.5 * (s * s)) / s;
        const double d_minus = d_plus - s;
        const double p_plus = fm_normal_cdf(d_plus);
        r.value = N * (F * p_plus - K * fm_normal_cdf(d_minus));
        r.delta = N * p_plus;
        r.vega = N * F * fm_normal_density(d_plus) * root_T;
    } else {
        const double d = (F - K) / s;
        const double p = fm_normal_cdf(d), q = fm_normal_density(d);
        r.value = N * ((F - K) * p + s * q);
        r.delta = N * p;
        r.vega = N * root_T * q;
    }
    return r;
}

} // namespace fmhost

// ---------------------------------------------------------------- host only: the argument checks and the definitions over arrays
#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdexcept>
#include <string>

namespace fmhost {

// what can be said about fmhip_function_apply's arguments without looking at a vector
inline void functionCheckApply(const int* kinds, int n_functions, const void* out)
{
    if (n_functions < 1 || n_functions > FM_FN_MAX_FUNCTIONS) throw std::invalid_argument("named functions: " + std::to_string(n_functions) + " functions in one call (1 … 4)");
    if (!kinds) throw std::invalid_argument("named functions: null pointer: kinds");
    if (!out) throw std::invalid_argument("named functions: null pointer: out");
    for (int f = 0; f < n_functions; ++f)
        if (kinds[f] < 0 || kinds[f] >= FM_FN_KINDS) throw std::invalid_argument("named functions: unknown function " + std::to_string(kinds[f]));
}
// … and about fmhip_option_formula's
inline void formulaCheck(int model, double maturity, double strike, int outputs, const void* out)
{
    if (model < 0 || model >= FM_FORMULA_MODELS) throw std::invalid_argument("option formula: unknown model " + std::to_string(model));
    if (!(maturity >= 0.0) || maturity - maturity != 0.0) throw std::invalid_argument("option formula: the maturity is finite and not negative");
    if (strike - strike != 0.0) throw std::invalid_argument("option formula: the strike is finite");
    if (outputs < 1 || outputs > FM_FORMULA_ALL) throw std::invalid_argument("option formula: outputs is a mask of value (1), delta (2) and vega (4)");
    if (!out) throw std::invalid_argument("option formula: null pointer: out");
}

inline void function_apply_host(const float* x, int64_t n, const int* kinds, int n_functions, float* const* out)
{
    functionCheckApply(kinds, n_functions, out);
    if (!x) throw std::invalid_argument("named functions: null pointer: x");
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("named functions: of " + std::to_string(n) + " elements (1 … 2^31)");
    for (int f = 0; f < n_functions; ++f) if (!out[f]) throw std::invalid_argument("named functions: null pointer: out[" + std::to_string(f) + "]");
    for (int64_t p = 0; p < n; ++p)
        for (int f = 0; f < n_functions; ++f) out[f][p] = fm_function_value(kinds[f], x[p]);
}

// forward, volatility, payoff_unit: an array of n floats, or NULL for the scalar beside it; out: one array per set bit of outputs, in bit order
inline void option_formula_host(int model, const float* forward, double forward_scalar, const float* volatility, double volatility_scalar,
                                const float* payoff_unit, double payoff_unit_scalar, int64_t n, double maturity, double strike, int outputs, float* const* out)
{
    formulaCheck(model, maturity, strike, outputs, out);
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("option formula: of " + std::to_string(n) + " elements (1 … 2^31)");
    const int n_out = fm_formula_outputs(outputs);
    for (int f = 0; f < n_out; ++f) if (!out[f]) throw std::invalid_argument("option formula: null pointer: out[" + std::to_string(f) + "]");
    const double root_T = __builtin_sqrt(maturity);
    for (int64_t p = 0; p < n; ++p) {
        const FmFormulaOut r = fm_option_formula(model, forward ? (double)forward[p] : forward_scalar, volatility ? (double)volatility[p] : volatility_scalar,
                                                 payoff_unit ? (double)payoff_unit[p] : payoff_unit_scalar, root_T, strike);
        int f = 0;
        if (outputs & FM_FORMULA_VALUE) out[f++][p] = fm_narrow(r.value);
        if (outputs & FM_FORMULA_DELTA) out[f++][p] = fm_narrow(r.delta);
        if (outputs & FM_FORMULA_VEGA) out[f++][p] = fm_narrow(r.vega);
    }
}

} // namespace fmhost
#endif
