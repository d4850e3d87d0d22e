// polynomial_regression.hpp — polynomial regression in one pass: the DEFINITION of the cross moments of a polynomial basis and of the fitted
// polynomial (include/fmhip.h: fmhip_polynomial_cross_moments_host, fmhip_polynomial_evaluate_host) and the ONE argument
// check both the host and the device entry points use (polynomialCheck*).  No device, no library: plain C++.
//
// A term is a monomial of up to 8 state vectors, exponents[n_terms][n_states], each 0 … 6.  u^e is u followed by e − 1 multiplications by u,
// each rounded to fp32: ((u·u)·u)…; the term is the product of the powers with e > 0 in ascending state index, left to right, each product
// rounded to fp32, nothing contracted.  A state with exponent 0 does not take part (it is not multiplied by 1: inf⁰ is no NaN); the all-zero
// tuple is the constant 1.0f.  The regressors are the terms in the order given, then the extra vectors (NULL / handle 0: the constant 1).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

constexpr int FM_POLY_MAX_STATES = 8;
constexpr int FM_POLY_MAX_EXPONENT = 6;
constexpr int FM_POLY_MAX_VECTORS = 64;            // terms, extra vectors and dependents of one moments call
constexpr int FM_POLY_MAX_EVAL = 60;               // terms and extra vectors of one evaluation

// T: a handle (0 = the constant 1) or a pointer (nullptr = the constant 1)
template <class T>
inline void polynomialCheckBasis(const T* states, int n_states, const uint8_t* exponents, int n_terms, const T* extra_x, int n_extra, const char* what) {
    const std::string w(what);
    if (n_states < 1 || n_states > FM_POLY_MAX_STATES) throw std::invalid_argument(w + " of " + std::to_string(n_states) + " state vectors: 1 … " + std::to_string(FM_POLY_MAX_STATES));
    if (n_terms < 1) throw std::invalid_argument(w + ": n_terms >= 1");
    if (n_extra < 0) throw std::invalid_argument(w + ": n_extra >= 0");
    if (!states || !exponents || (n_extra > 0 && !extra_x)) throw std::invalid_argument(w + ": a required pointer is NULL");
    for (int s = 0; s < n_states; ++s) if (!states[s]) throw std::invalid_argument(w + ": a state is a vector, not the constant 1");
    for (int i = 0; i < n_terms * n_states; ++i)
        if (exponents[i] > FM_POLY_MAX_EXPONENT) throw std::invalid_argument(w + ": exponent " + std::to_string((int)exponents[i]) + " above " + std::to_string(FM_POLY_MAX_EXPONENT));
}
template <class T>
inline void polynomialCheckMoments(const T* states, int n_states, const uint8_t* exponents, int n_terms, const T* extra_x, int n_extra, const T* y, int n_y, const void* sums_out) {
    if (n_y < 0) throw std::invalid_argument("polynomial cross moments: n_y >= 0");
    if (n_terms > FM_POLY_MAX_VECTORS || n_extra > FM_POLY_MAX_VECTORS || n_y > FM_POLY_MAX_VECTORS || (n_terms > 0 ? n_terms : 0) + (n_extra > 0 ? n_extra : 0) + n_y > FM_POLY_MAX_VECTORS)
        throw std::invalid_argument("polynomial cross moments of " + std::to_string(n_terms) + " + " + std::to_string(n_extra) + " + " + std::to_string(n_y) + " regressors and dependents: at most " + std::to_string(FM_POLY_MAX_VECTORS));
    polynomialCheckBasis<T>(states, n_states, exponents, n_terms, extra_x, n_extra, "polynomial cross moments");
    if ((n_y > 0 && !y) || !sums_out) throw std::invalid_argument("polynomial cross moments: a required pointer is NULL");
    for (int m = 0; m < n_y; ++m) if (!y[m]) throw std::invalid_argument("the constant 1 is a regressor, not a dependent");
}
template <class T>
inline void polynomialCheckEvaluate(const T* states, int n_states, const uint8_t* exponents, int n_terms, const T* extra_x, int n_extra, const double* coefficients, const void* out) {
    if (n_terms > FM_POLY_MAX_EVAL || n_extra > FM_POLY_MAX_EVAL || (n_terms > 0 ? n_terms : 0) + (n_extra > 0 ? n_extra : 0) > FM_POLY_MAX_EVAL)
        throw std::invalid_argument("polynomial evaluation of " + std::to_string(n_terms) + " + " + std::to_string(n_extra) + " regressors: at most " + std::to_string(FM_POLY_MAX_EVAL));
    polynomialCheckBasis<T>(states, n_states, exponents, n_terms, extra_x, n_extra, "polynomial evaluation");
    if (!coefficients || !out) throw std::invalid_argument("polynomial evaluation: a required pointer is NULL");
}

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
// one term on one path; u[s]: the states' values there
inline float polynomialTerm(const float* u, int n_states, const uint8_t* e) {
    bool started = false;
    volatile float t = 1.0f;
    for (int s = 0; s < n_states; ++s) {
        if (!e[s]) continue;
        volatile float p = u[s];
        for (int j = 1; j < (int)e[s]; ++j) p = p * u[s];
        if (started) t = t * p; else t = p;
        started = true;
    }
    return t;
}
// r = ((t_0·c_0) + t_1·c_1) + … over the terms, then the extra vectors; c_i = (float)coefficients[i]
inline void polynomialEvaluate(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms, const float* const* extra_x, int n_extra,
                               const double* coefficients, float* out) {
    polynomialCheckEvaluate<const float*>(states, n_states, exponents, n_terms, extra_x, n_extra, coefficients, out);
    if (n <= 0) throw std::invalid_argument("polynomial evaluation of an empty vector");
    for (int64_t p = 0; p < n; ++p) {
        float u[FM_POLY_MAX_STATES];
        for (int s = 0; s < n_states; ++s) u[s] = states[s][p];
        volatile float r = polynomialTerm(u, n_states, exponents) * (float)coefficients[0];
        for (int i = 1; i < n_terms; ++i) { volatile float t = polynomialTerm(u, n_states, exponents + (size_t)i * n_states) * (float)coefficients[i]; r = r + t; }
        for (int j = 0; j < n_extra; ++j) { volatile float t = (extra_x[j] ? extra_x[j][p] : 1.0f) * (float)coefficients[n_terms + j]; r = r + t; }
        out[p] = r;
    }
}
#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

// sums_out: S packed upper triangle (row-major) of the n_x = n_terms + n_extra regressors, then T[i·n_y + m] — fmhip_cross_moments' layout.
// Every product of two floats is exact in fp64; the paths are added in path order.
inline void polynomialCrossMoments(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms, const float* const* extra_x, int n_extra,
                                   const float* const* y, int n_y, double* sums_out) {
    polynomialCheckMoments<const float*>(states, n_states, exponents, n_terms, extra_x, n_extra, y, n_y, sums_out);
    if (n <= 0) throw std::invalid_argument("polynomial cross moments of an empty vector");
    const int n_x = n_terms + n_extra;
    const size_t q = (size_t)n_x * (n_x + 1) / 2 + (size_t)n_x * n_y;
    for (size_t i = 0; i < q; ++i) sums_out[i] = 0.0;
    std::vector<double> xv((size_t)n_x), yv((size_t)n_y);
    for (int64_t p = 0; p < n; ++p) {
        float u[FM_POLY_MAX_STATES];
        for (int s = 0; s < n_states; ++s) u[s] = states[s][p];
        for (int i = 0; i < n_terms; ++i) xv[(size_t)i] = (double)polynomialTerm(u, n_states, exponents + (size_t)i * n_states);
        for (int j = 0; j < n_extra; ++j) xv[(size_t)(n_terms + j)] = extra_x[j] ? (double)extra_x[j][p] : 1.0;
        for (int m = 0; m < n_y; ++m) yv[(size_t)m] = (double)y[m][p];
        double* s = sums_out;
        for (int i = 0; i < n_x; ++i) for (int j = i; j < n_x; ++j) *s++ += xv[(size_t)i] * xv[(size_t)j];
        for (int i = 0; i < n_x; ++i) for (int m = 0; m < n_y; ++m) *s++ += xv[(size_t)i] * yv[(size_t)m];
    }
}

} // namespace fmhost
