// resample_host.hpp — the DEFINITION of the device resampling (fmhip_resample_host), compiled by the host AND by the kernels
// (resample_kernel.hip): the cleaning of a weight, the uniform in force, the fraction, the target and the search are ONE function each, so the
// device's ancestors are the host's bit for bit.  No HIP beyond the __host__ __device__ marks and no libm; fp64, every operation rounded on
// its own (-ffp-contract=off, as everywhere).  tests/cpp/test_resample_host.cpp drives it, sanitized, on the CPU.
//
// m ancestors are drawn from n weights and up to 8 companion vectors are carried along: out[i][j] = values[i][a_j].
//   cleaned weight   cw[r] = w[r] if w[r] > 0, otherwise +0.0: a NaN, a negative weight and -0.0 count as zero.
//   P, total         P = the prefix sums of cw in the tree of prefix_host.hpp (non-decreasing: cw has no NaN and nothing negative), total =
//                    P[n-1].  Without a weight vector P[r] = (double)(r + 1) and total = (double)n: nothing is summed, nothing searched.
//   degenerate       !(total > 0) or total == +inf: every output element is the quiet NaN 0x7fc00000, every ancestor NaN (host twin: -1).
//   U_j              (double)u[j]; below 0 it is 0, at or above 1 it is the largest double below 1; a NaN makes element j DEAD (as degenerate).
//   f_j              SYSTEMATIC ((double)j + offset) / (double)m; STRATIFIED ((double)j + U_j) / (double)m; MULTINOMIAL U_j.
//   t_j              fl(f_j · total), one rounding.  0 <= f_j <= 1 (the sum (double)j + U can round up to m), so 0 <= t_j <= total.
//   a_j              the smallest r with P[r] > t_j; if there is none — t_j == total, which only rounding at the top can cause — the smallest
//                    r with P[r] == total.  Both in one monotone predicate: the smallest r with  P[r] > t_j || P[r] >= total  (while
//                    t_j < total the first r with P[r] > t_j comes no later than the first with P[r] == total).
// Two consequences, both tested:
//   cw[a_j] > 0 always — P[a_j] > P[a_j - 1] (or a_j = 0 and P[0] > 0), and a zero weight repeats the prefix before it bit for bit at every
//                    level of the tree: a path of zero weight is never an ancestor, at t = 0 as little as anywhere;
//   0 <= a_j <= n-1 always — P[n-1] >= total holds, so the predicate is true at n - 1 whatever t_j is.
// With equal weights a_j = min((int64)t_j, n - 1): the bootstrap.
#pragma once
#include "prefix_host.hpp"

#include <cstring>
#include <vector>

#if defined(__HIP__)
#define FM_RESAMPLE_HD __host__ __device__ __forceinline__
#else
#define FM_RESAMPLE_HD inline
#endif

namespace fm {

constexpr int FM_RESAMPLE_SYSTEMATIC = 0, FM_RESAMPLE_STRATIFIED = 1, FM_RESAMPLE_MULTINOMIAL = 2;      // FMHIP_RESAMPLE_*
constexpr int FM_RESAMPLE_MAX_VALUES = 8;
constexpr int64_t FM_RESAMPLE_MAX_ANCESTOR_N = int64_t(1) << 24;       // (float)a_j is exact up to here
constexpr uint32_t FM_RESAMPLE_NAN_BITS = 0x7fc00000u;

FM_RESAMPLE_HD bool resample_needs_uniforms(int scheme) { return scheme != FM_RESAMPLE_SYSTEMATIC; }
FM_RESAMPLE_HD float resample_clean(float w) { return w > 0.0f ? w : 0.0f; }
FM_RESAMPLE_HD bool resample_degenerate(double total) { return !(total > 0.0) || total == __builtin_inf(); }
// U_j; false: the element is dead
FM_RESAMPLE_HD bool resample_uniform(float u, double& U)
{
    const double x = (double)u;
    if (x != x) { U = 0.0; return false; }
    U = x < 0.0 ? 0.0 : x >= 1.0 ? 0x1.fffffffffffffp-1 : x;
    return true;
}
FM_RESAMPLE_HD double resample_fraction(int scheme, int64_t j, int64_t m, double offset, double U)
{
    if (scheme == FM_RESAMPLE_MULTINOMIAL) return U;
    return ((double)j + (scheme == FM_RESAMPLE_SYSTEMATIC ? offset : U)) / (double)m;
}
FM_RESAMPLE_HD double resample_target(double f, double total) { return f * total; }
// a_j with equal weights (t >= 0)
FM_RESAMPLE_HD int64_t resample_equal_ancestor(double t, int64_t n)
{
    const int64_t a = (int64_t)t;
    return a < n - 1 ? a : n - 1;
}
// the trips of resample_search over `len` elements: the bit length of len, a function of the size alone
FM_RESAMPLE_HD int resample_trips(int64_t len)
{
    int trips = 0;
    for (; len > 0; len >>= 1) ++trips;
    return trips;
}
// The smallest r in [lo, lo + len) with  p[r] > t || p[r] >= total, or lo + len: a bisection of EXACTLY `trips` steps (>= resample_trips(len);
// a step on an empty range changes nothing) whose every load address is clamped into [0, last] before the load — no value of p, t or total
// can make it read elsewhere or run longer.  p non-decreasing.  One step (the kernel runs the steps of a lane's outputs side by side):
FM_RESAMPLE_HD void resample_search_step(const double* p, int64_t& lo, int64_t& len, int64_t last, double t, double total)
{
    const int64_t half = len >> 1;
    int64_t mid = lo + half;
    mid = mid < 0 ? 0 : mid > last ? last : mid;
    const double x = p[mid];
    const bool hit = x > t || x >= total;
    if (len > 0 && !hit) { lo = lo + half + 1; len = len - half - 1; }
    else len = half;
}
FM_RESAMPLE_HD int64_t resample_search(const double* p, int64_t lo, int64_t len, int trips, int64_t last, double t, double total)
{
    for (int it = 0; it < trips; ++it) resample_search_step(p, lo, len, last, t, total);
    return lo;
}

inline bool resample_scheme_ok(int scheme) { return scheme == FM_RESAMPLE_SYSTEMATIC || scheme == FM_RESAMPLE_STRATIFIED || scheme == FM_RESAMPLE_MULTINOMIAL; }
// what can be said about the scalars of a call (std::invalid_argument, as the other definitions complain)
inline void resample_check_scalars(int scheme, int64_t m, double offset, int n_values, bool want_ancestors, bool have_weights, bool have_uniforms)
{
    if (!resample_scheme_ok(scheme)) throw std::invalid_argument("resample: scheme " + std::to_string(scheme) + " (FMHIP_RESAMPLE_SYSTEMATIC, _STRATIFIED or _MULTINOMIAL)");
    if (!prefix_size_ok(m)) throw std::invalid_argument("resample: " + std::to_string(m) + " outputs: 1 … 2^31 - 1");
    if (n_values < 0 || n_values > FM_RESAMPLE_MAX_VALUES) throw std::invalid_argument("resample: " + std::to_string(n_values) + " value vectors: 0 … " + std::to_string(FM_RESAMPLE_MAX_VALUES));
    if (n_values == 0 && !want_ancestors) throw std::invalid_argument("resample: nothing asked for: no value vector and no ancestors_out");
    if (n_values == 0 && !have_weights) throw std::invalid_argument("resample: neither weights nor a value vector");
    if (!(offset >= 0.0 && offset < 1.0)) throw std::invalid_argument("resample: the offset is in [0, 1)");      // (whatever the scheme: 0 where it is not read)
    if (resample_needs_uniforms(scheme) && !have_uniforms) throw std::invalid_argument("resample: this scheme needs uniforms");
}
inline void resample_check_size(int64_t n, bool want_ancestors)
{
    if (!prefix_size_ok(n)) throw std::invalid_argument("resample from " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    if (want_ancestors && n > FM_RESAMPLE_MAX_ANCESTOR_N) throw std::invalid_argument("resample: ancestors_out is offered up to 2^24 elements, where the float is exact");
}

// The definition.  weights: n floats or null (equal weights); uniforms: m floats (not read with SYSTEMATIC); values / values_out: n_values
// pointers to n resp. m floats; ancestors_out (m, -1 for a dead element) and total_out may be null.
inline void resample_host(const float* weights, int64_t n, int scheme, int64_t m, double offset, const float* uniforms, const float* const* values, int n_values,
                          float* const* values_out, int64_t* ancestors_out, double* total_out)
{
    resample_check_scalars(scheme, m, offset, n_values, ancestors_out != nullptr, weights != nullptr, uniforms != nullptr);
    resample_check_size(n, ancestors_out != nullptr);
    if (n_values > 0 && (!values || !values_out)) throw std::invalid_argument("resample: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i] || !values_out[i]) throw std::invalid_argument("resample: null pointer");
    std::vector<double> P;
    double total = (double)n;
    if (weights) {
        std::vector<float> cw((size_t)n);
        for (int64_t r = 0; r < n; ++r) cw[(size_t)r] = resample_clean(weights[r]);
        P.resize((size_t)n);
        prefix_sums_host(cw.data(), n, P.data());
        total = P[(size_t)n - 1];
    }
    if (total_out) *total_out = total;
    const bool degenerate = resample_degenerate(total);
    const int trips = resample_trips(n);
    for (int64_t j = 0; j < m; ++j) {
        double U = 0.0;
        const bool alive = !degenerate && (!resample_needs_uniforms(scheme) || resample_uniform(uniforms[j], U));
        int64_t a = -1;
        if (alive) {
            const double t = resample_target(resample_fraction(scheme, j, m, offset, U), total);
            a = weights ? resample_search(P.data(), 0, n, trips, n - 1, t, total) : resample_equal_ancestor(t, n);
            a = a < 0 ? 0 : a > n - 1 ? n - 1 : a;
        }
        if (ancestors_out) ancestors_out[j] = a;
        for (int i = 0; i < n_values; ++i) {
            if (a >= 0) std::memcpy(&values_out[i][j], &values[i][a], 4);
            else std::memcpy(&values_out[i][j], &FM_RESAMPLE_NAN_BITS, 4);
        }
    }
}

} // namespace fm
