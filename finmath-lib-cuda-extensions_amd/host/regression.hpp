// regression.hpp — least-squares regression over the common RandomVariable interface (random_variable.hpp): the pivoted Cholesky of the
// normal equations and the conditional-expectation estimator finmath-lib's American Monte-Carlo code is written against
// (net.finmath.montecarlo.conditionalexpectation.MonteCarloConditionalExpectationRegression).  The C++ twin of regression.py: the same
// pivot rule step for step, the same two ways to the normal equations — ONE fmhip_cross_moments call (include/fmhip.h)
// when every stochastic operand has a device vector, b_i.mult(b_j).getAverage() pair by pair otherwise or with FMHIP_DEVICE_CROSS_MOMENTS=0.
// FMHOST_REGRESSION_SOLVER_ONLY: the solver alone, without the interface (a build without the library).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <vector>

namespace fmhost {

// x with A x = b in the least-squares sense; A symmetric positive SEMI-definite, K x K row-major; b and x: K x M row-major.  Cholesky with
// diagonal pivoting: the largest remaining pivot next (the first of equals); once it is <= 1e-12 x the largest diagonal entry of A the
// remaining unknowns are 0 — a collinear basis function, the indicator of an empty bin.
inline std::vector<double> solveNormalEquations(const std::vector<double>& A, const std::vector<double>& b, int K, int M = 1) {
    std::vector<int> perm((size_t)K);
    std::vector<double> d((size_t)K), L((size_t)K * K, 0.0), x((size_t)K * M, 0.0);
    double largest = 0.0;
    for (int i = 0; i < K; ++i) { perm[(size_t)i] = i; d[(size_t)i] = A[(size_t)i * K + i]; if (i == 0 || d[(size_t)i] > largest) largest = d[(size_t)i]; }
    const double tol = 1e-12 * largest;
    int rank = K;
    for (int k = 0; k < K; ++k) {
        int p = k;
        for (int q = k + 1; q < K; ++q) if (d[(size_t)perm[(size_t)q]] > d[(size_t)perm[(size_t)p]]) p = q;
        if (d[(size_t)perm[(size_t)p]] <= tol) { rank = k; break; }
        std::swap(perm[(size_t)k], perm[(size_t)p]);
        const int i = perm[(size_t)k];
        L[(size_t)i * K + k] = std::sqrt(d[(size_t)i]);
        for (int q = k + 1; q < K; ++q) {
            const int j = perm[(size_t)q];
            double s = A[(size_t)j * K + i];
            for (int t = 0; t < k; ++t) s -= L[(size_t)j * K + t] * L[(size_t)i * K + t];
            L[(size_t)j * K + k] = s / L[(size_t)i * K + k];
            d[(size_t)j] -= L[(size_t)j * K + k] * L[(size_t)j * K + k];
        }
    }
    std::vector<double> z((size_t)rank);
    for (int m = 0; m < M; ++m) {
        for (int k = 0; k < rank; ++k) {            // L z = b
            double s = b[(size_t)perm[(size_t)k] * M + m];
            for (int t = 0; t < k; ++t) s -= L[(size_t)perm[(size_t)k] * K + t] * z[(size_t)t];
            z[(size_t)k] = s / L[(size_t)perm[(size_t)k] * K + k];
        }
        for (int k = rank - 1; k >= 0; --k) {       // Lᵀ x = z
            double s = z[(size_t)k];
            for (int t = k + 1; t < rank; ++t) s -= L[(size_t)perm[(size_t)t] * K + k] * x[(size_t)perm[(size_t)t] * M + m];
            x[(size_t)perm[(size_t)k] * M + m] = s / L[(size_t)perm[(size_t)k] * K + k];
        }
    }
    return x;
}

} // namespace fmhost

#ifndef FMHOST_REGRESSION_SOLVER_ONLY
#include "random_variable.hpp"

namespace fmhost {

class MonteCarloConditionalExpectationRegression {
public:
    explicit MonteCarloConditionalExpectationRegression(std::vector<RV> basisFunctionsEstimator, std::vector<RV> basisFunctionsPredictor = {})
        : estimator_(std::move(basisFunctionsEstimator)), predictor_(basisFunctionsPredictor.empty() ? estimator_ : std::move(basisFunctionsPredictor)) {
        if (predictor_.size() != estimator_.size()) throw std::invalid_argument("estimator and predictor need the same number of basis functions");
    }
    static bool deviceCrossMoments() { const char* e = std::getenv("FMHIP_DEVICE_CROSS_MOMENTS"); return !(e && e[0] == '0' && e[1] == 0); }

    std::vector<double> getLinearRegressionParameters(const RV& dependent) const {
        const int K = (int)estimator_.size();
        std::vector<double> A((size_t)K * K), b((size_t)K);
        if (!normalEquationsOnePass(dependent, A, b)) {
            for (int i = 0; i < K; ++i) {
                for (int j = i; j < K; ++j) A[(size_t)i * K + j] = A[(size_t)j * K + i] = estimator_[(size_t)i]->mult(estimator_[(size_t)j])->getAverage();
                b[(size_t)i] = estimator_[(size_t)i]->mult(dependent)->getAverage();
            }
        }
        return solveNormalEquations(A, b, K);
    }
    // Σ β_i·b_i over the predictor's basis functions, built with mult / addProduct as finmath-lib builds it
    RV getConditionalExpectation(const RV& dependent) const {
        const std::vector<double> beta = getLinearRegressionParameters(dependent);
        RV ce = predictor_[0]->mult(beta[0]);
        for (size_t i = 1; i < predictor_.size(); ++i) ce = ce->addProduct(predictor_[i], beta[i]);
        return ce;
    }

private:
    // the one-pass path: every stochastic operand has a device vector (orderStatisticsHandle), deterministic basis functions are host
    // scalars folded through the constant-1 entry (c·Σx_j, c·c'·n)
    bool normalEquationsOnePass(const RV& dependent, std::vector<double>& A, std::vector<double>& b) const {
        const int K = (int)estimator_.size();
        // up to 12 basis functions: fmhip_cross_moments and its bits; up to 60: fmhip_cross_moments_wide, unless
        // FMHIP_DEVICE_WIDE_MOMENTS=0 (read per call) sends them pair by pair
        const bool wide = K > 12;
        if (wide) { const char* knob = std::getenv("FMHIP_DEVICE_WIDE_MOMENTS"); if (knob && knob[0] == '0' && knob[1] == 0) return false; }
        if (!deviceCrossMoments() || K < 1 || K > 60 || dependent->isDeterministic() || !dependent->orderStatisticsHandle()) return false;
        std::vector<fmhip_vec> x((size_t)K);
        std::vector<double> scale((size_t)K, 1.0);
        const RandomVariable* sized = nullptr;
        for (int i = 0; i < K; ++i) {
            const RV& f = estimator_[(size_t)i];
            if (f->isDeterministic()) {
                if (!dynamic_cast<const RandomVariableHip*>(f.get())) return false;
                x[(size_t)i] = 0; scale[(size_t)i] = f->doubleValue();
            } else if ((x[(size_t)i] = f->orderStatisticsHandle()) != 0) sized = f.get();
            else return false;
        }
        if (!sized) return false;
        const fmhip_vec y = dependent->orderStatisticsHandle();
        std::vector<double> sums((size_t)K * (K + 1) / 2 + (size_t)K);
        check(wide ? fmhip_cross_moments_wide(x.data(), K, &y, 1, sums.data()) : fmhip_cross_moments(x.data(), K, &y, 1, sums.data()));
        const double n = (double)sized->sampleSize();
        size_t at = 0;
        for (int i = 0; i < K; ++i) for (int j = i; j < K; ++j, ++at) A[(size_t)i * K + j] = A[(size_t)j * K + i] = sums[at] * (scale[(size_t)i] * scale[(size_t)j]) / n;
        for (int i = 0; i < K; ++i) b[(size_t)i] = sums[at + (size_t)i] * scale[(size_t)i] / n;
        return true;
    }
    std::vector<RV> estimator_, predictor_;
};

} // namespace fmhost
#endif
