// localized_regression.hpp — the C++ twin of regression.py's MonteCarloConditionalExpectationLocalizedRegression over the common RandomVariable
// interface (random_variable.hpp): a least-squares fit per bin of a key, the block-diagonal normal equations from ONE
// fmhip_binned_cross_moments call and the piecewise estimate from ONE fmhip_binned_evaluate call (include/fmhip.h), each
// block solved by regression.hpp's pivoted Cholesky (an empty bin gets coefficients 0).  Every stochastic operand has a device vector and
// there are at most three basis functions (limits, bin rule and argument checks: binned_regression.hpp, which the host entry points use
// too); the generic path over any RandomVariable class is the Python mirror's.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "binned_regression.hpp"
#include "regression.hpp"

namespace fmhost {

class MonteCarloConditionalExpectationLocalizedRegression {
public:
    // bounds: n_bins - 1 ascending values; empty: bins of equal count, sorted(key)[ceil(j n / n_bins) - 1] from one fmhip_select_ranks_batch call
    MonteCarloConditionalExpectationLocalizedRegression(RV key, int n_bins, std::vector<RV> basisFunctionsEstimator, std::vector<RV> basisFunctionsPredictor = {}, std::vector<double> bounds = {})
        : key_(std::move(key)), n_bins_(n_bins), estimator_(std::move(basisFunctionsEstimator)), predictor_(basisFunctionsPredictor.empty() ? estimator_ : std::move(basisFunctionsPredictor)), bounds_(std::move(bounds)) {
        if (n_bins_ < 1 || n_bins_ > FM_BINNED_MAX_BINS) throw std::invalid_argument("n_bins must be 1 … 64");
        if (predictor_.size() != estimator_.size() || estimator_.empty() || (int)estimator_.size() > FM_BINNED_MAX_X) throw std::invalid_argument("estimator and predictor need the same number of basis functions, 1 … 3");
        if (key_->isDeterministic() || !key_->orderStatisticsHandle()) throw std::invalid_argument("the key is a stochastic random variable with a device vector");
        if (bounds_.empty() && n_bins_ > 1) {
            const int64_t n = (int64_t)key_->sampleSize();
            std::vector<int64_t> ranks;
            for (int j = 1; j < n_bins_; ++j) ranks.push_back(std::max<int64_t>(((int64_t)j * n + n_bins_ - 1) / n_bins_ - 1, 0));
            bounds_.resize(ranks.size());
            const fmhip_vec h = key_->orderStatisticsHandle();
            check(fmhip_select_ranks_batch(&h, 1, ranks.data(), (int)ranks.size(), bounds_.data()));
        }
        if ((int)bounds_.size() != n_bins_ - 1) throw std::invalid_argument("n_bins bins have n_bins - 1 bounds");
        binnedCheckBins(bounds_.data(), n_bins_);                  // the check of the entry points: ascending, no NaN
    }
    const std::vector<double>& bounds() const { return bounds_; }

    // beta[bin * K + i]
    std::vector<double> getLinearRegressionParameters(const RV& dependent) const {
        const int K = (int)estimator_.size(), q = binnedSumsPerBin(K, 1);
        std::vector<double> scale((size_t)K, 1.0);
        const std::vector<fmhip_vec> x = handles(estimator_, &scale);
        const fmhip_vec y = dependent->isDeterministic() ? 0 : dependent->orderStatisticsHandle();
        if (!y) throw std::invalid_argument("the dependent is a stochastic random variable with a device vector");
        std::vector<int64_t> counts((size_t)n_bins_);
        std::vector<double> sums((size_t)n_bins_ * q), beta((size_t)n_bins_ * K);
        check(fmhip_binned_cross_moments(key_->orderStatisticsHandle(), bounds_.data(), n_bins_, x.data(), K, &y, 1, counts.data(), sums.data()));
        const double n = (double)key_->sampleSize();
        for (int b = 0; b < n_bins_; ++b) {
            std::vector<double> A((size_t)K * K), t((size_t)K);
            size_t at = (size_t)b * q;
            for (int i = 0; i < K; ++i) for (int j = i; j < K; ++j, ++at) A[(size_t)i * K + j] = A[(size_t)j * K + i] = sums[at] * (scale[(size_t)i] * scale[(size_t)j]) / n;
            for (int i = 0; i < K; ++i) t[(size_t)i] = sums[at + (size_t)i] * scale[(size_t)i] / n;
            const std::vector<double> one = solveNormalEquations(A, t, K);
            std::copy(one.begin(), one.end(), beta.begin() + (size_t)b * K);
        }
        return beta;
    }
    // the handle of a new vector: per path the fit of its bin, in the fp32 arithmetic of basis[0].mult(β0).addProduct(basis[i], βi); the caller releases it
    fmhip_vec getConditionalExpectationHandle(const RV& dependent) const {
        const std::vector<double> beta = getLinearRegressionParameters(dependent);
        const std::vector<fmhip_vec> x = handles(predictor_, nullptr);
        fmhip_vec out = 0;
        check(fmhip_binned_evaluate(key_->orderStatisticsHandle(), bounds_.data(), n_bins_, x.data(), (int)x.size(), beta.data(), &out));
        return out;
    }

private:
    // deterministic basis functions are the constant 1 (handle 0), scaled on the host in the normal equations; a predictor's must BE 1
    static std::vector<fmhip_vec> handles(const std::vector<RV>& functions, std::vector<double>* scale) {
        std::vector<fmhip_vec> x(functions.size(), 0);
        for (size_t i = 0; i < functions.size(); ++i) {
            const RV& f = functions[i];
            if (f->isDeterministic()) {
                if (scale) (*scale)[i] = f->doubleValue();
                else if (f->doubleValue() != 1.0) throw std::invalid_argument("a deterministic predictor is the constant 1");
            } else if (!(x[i] = f->orderStatisticsHandle())) throw std::invalid_argument("every stochastic basis function has a device vector");
        }
        return x;
    }
    RV key_;
    int n_bins_;
    std::vector<RV> estimator_, predictor_;
    std::vector<double> bounds_;
};

} // namespace fmhost
