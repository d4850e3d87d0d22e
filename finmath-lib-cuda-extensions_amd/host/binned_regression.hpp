// binned_regression.hpp — localized regression: the DEFINITION of the binned cross moments and of the piecewise evaluation (include/fmhip.h:
// fmhip_binned_cross_moments_host, fmhip_binned_evaluate_host), the ONE argument check both the host and the device entry
// points use (binnedCheck*).  The C++ mirror of regression.py's localized estimator (localized_regression.hpp) includes this header for
// the limits and the checks.  No device, no library: plain C++.
//
// Bins.  bounds[n_bins - 1] non-decreasing doubles, ±inf allowed, no NaN; bin(k) = #{ j : bounds[j] < (double)k } — k lies in bin j iff
// bounds[j-1] < k <= bounds[j], the comparison of fmhip_count_not_above (so -0.0 and +0.0 fall on the same side of a bound of 0).  A NaN
// key belongs to no bin.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

constexpr int FM_BINNED_MAX_BINS = 64;
constexpr int FM_BINNED_MAX_X = 3;
constexpr int FM_BINNED_MAX_Y = 4;

// -1 for a NaN key; the search is the device's: six levels over bounds padded with +inf, no branch on the data
inline int binnedBinOf(float key, const double* bounds, int n_bins) {
    if (key != key) return -1;
    const double k = (double)key;
    int pos = 0;
    for (int half = 32; half != 0; half >>= 1) {
        const int t = pos + half;
        if (t <= n_bins - 1 && bounds[t - 1] < k) pos = t;
    }
    return pos;
}

// What can be said about the bins without looking at a vector.  T: a handle (0 = the constant 1) or a pointer (nullptr = the constant 1).
inline void binnedCheckBins(const double* bounds, int n_bins) {
    if (n_bins < 1 || n_bins > FM_BINNED_MAX_BINS) throw std::invalid_argument("binned pass over " + std::to_string(n_bins) + " bins: 1 … " + std::to_string(FM_BINNED_MAX_BINS));
    if (n_bins > 1 && !bounds) throw std::invalid_argument("binned pass: bounds is NULL");
    for (int j = 0; j + 1 < n_bins; ++j) {
        if (bounds[j] != bounds[j]) throw std::invalid_argument("binned pass: a bound is NaN");
        if (j > 0 && bounds[j] < bounds[j - 1]) throw std::invalid_argument("binned pass: the bounds are not sorted");
    }
}
template <class T>
inline void binnedCheckMoments(T key, const double* bounds, int n_bins, const T* x, int n_x, const T* y, int n_y, const void* counts_out, const void* sums_out) {
    if (n_x < 1 || n_x > FM_BINNED_MAX_X) throw std::invalid_argument("binned cross moments of " + std::to_string(n_x) + " vectors: 1 … " + std::to_string(FM_BINNED_MAX_X));
    if (n_y < 0 || n_y > FM_BINNED_MAX_Y) throw std::invalid_argument("binned cross moments with " + std::to_string(n_y) + " dependents: 0 … " + std::to_string(FM_BINNED_MAX_Y));
    if (!x || (n_y > 0 && !y) || !counts_out || !sums_out) throw std::invalid_argument("binned cross moments: a required pointer is NULL");
    if (!key) throw std::invalid_argument("binned cross moments: the key is a vector, not the constant 1");
    for (int m = 0; m < n_y; ++m) if (!y[m]) throw std::invalid_argument("the constant 1 is an x, not a y");
    binnedCheckBins(bounds, n_bins);
}
template <class T>
inline void binnedCheckEvaluate(T key, const double* bounds, int n_bins, const T* x, int n_x, const double* coefficients, const void* out) {
    if (n_x < 1 || n_x > FM_BINNED_MAX_X) throw std::invalid_argument("binned evaluation of " + std::to_string(n_x) + " vectors: 1 … " + std::to_string(FM_BINNED_MAX_X));
    if (!x || !coefficients || !out) throw std::invalid_argument("binned evaluation: a required pointer is NULL");
    if (!key) throw std::invalid_argument("binned evaluation: the key is a vector, not the constant 1");
    binnedCheckBins(bounds, n_bins);
}

inline int binnedSumsPerBin(int n_x, int n_y) { return n_x * (n_x + 1) / 2 + n_x * n_y; }

// counts_out[n_bins]; sums_out[n_bins][q], q = n_x(n_x+1)/2 + n_x·n_y: S packed upper triangle (row-major), then T[i·n_y + m] — the layout
// of fmhip_cross_moments per bin.  Every product of two floats is exact in fp64; a bin's members are added in path order.
inline void binnedCrossMoments(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x, const float* const* y, int n_y,
                               int64_t* counts_out, double* sums_out) {
    binnedCheckMoments<const float*>(key, bounds, n_bins, x, n_x, y, n_y, counts_out, sums_out);
    if (n <= 0) throw std::invalid_argument("binned cross moments of an empty vector");
    const int q = binnedSumsPerBin(n_x, n_y);
    for (int b = 0; b < n_bins; ++b) counts_out[b] = 0;
    for (size_t i = 0; i < (size_t)n_bins * q; ++i) sums_out[i] = 0.0;
    for (int64_t p = 0; p < n; ++p) {
        const int b = binnedBinOf(key[p], bounds, n_bins);
        if (b < 0) continue;
        ++counts_out[b];
        double xv[FM_BINNED_MAX_X], yv[FM_BINNED_MAX_Y];
        for (int i = 0; i < n_x; ++i) xv[i] = x[i] ? (double)x[i][p] : 1.0;
        for (int m = 0; m < n_y; ++m) yv[m] = (double)y[m][p];
        double* s = sums_out + (size_t)b * q;
        for (int i = 0; i < n_x; ++i) for (int j = i; j < n_x; ++j) *s++ += xv[i] * xv[j];
        for (int i = 0; i < n_x; ++i) for (int m = 0; m < n_y; ++m) *s++ += xv[i] * yv[m];
    }
}

// out[p] = ((x_0[p]·c_0) + x_1[p]·c_1) + …, c_i = (float)coefficients[bin(key[p])·n_x + i]: every product and every sum rounded to fp32,
// nothing contracted — what basis[0].mult(β0).addProduct(basis[i], βi) computes.  The constant 1 is 1.0f; a NaN key gives NaN.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
inline float binnedEvaluateOne(int bin, const float* xv, int n_x, const double* coefficients) {
    if (bin < 0) return std::numeric_limits<float>::quiet_NaN();
    const double* c = coefficients + (size_t)bin * n_x;
    volatile float r = xv[0] * (float)c[0];
    for (int i = 1; i < n_x; ++i) { volatile float t = xv[i] * (float)c[i]; r = r + t; }
    return r;
}
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif
inline void binnedEvaluate(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x, const double* coefficients, float* out) {
    binnedCheckEvaluate<const float*>(key, bounds, n_bins, x, n_x, coefficients, out);
    if (n <= 0) throw std::invalid_argument("binned evaluation of an empty vector");
    for (int64_t p = 0; p < n; ++p) {
        float xv[FM_BINNED_MAX_X];
        for (int i = 0; i < n_x; ++i) xv[i] = x[i] ? x[i][p] : 1.0f;
        out[p] = binnedEvaluateOne(binnedBinOf(key[p], bounds, n_bins), xv, n_x, coefficients);
    }
}

} // namespace fmhost
