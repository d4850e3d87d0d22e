// independent_increments.hpp — finmath-lib's IndependentIncrementsFromICDF in the C++ host mirror: increments with a law per (time step,
// factor) drawn from the MT19937 stream through an inverse CDF (host/increments.hpp is the definition) [unverified: finmath-lib is not
// vendored; the class name, the draw order and the Merton layout are restated from its documentation].
//   IndependentIncrementsFromICDF      draws on the host and hands every increment to the injected factory, like
//                                      BrownianMotionFromMersenneRandomNumbers: every back end sees the same numbers
//   IndependentIncrementsFromICDFHip   the same numbers GENERATED ON THE DEVICE (fmhip_increments_generate_device), with a path offset
// Both implement BrownianMotion (whose getIncrement is the IndependentIncrements method), so a driver written against it takes them.
#pragma once
#include <functional>
#include <mutex>

#include "increments.hpp"
#include "random_variable.hpp"

namespace fmhost {

struct Law {
    int32_t kind; double a, b;
    static Law normal(double scale) { return { LAW_NORMAL, scale, 0.0 }; }
    static Law uniform(double lo, double hi) { return { LAW_UNIFORM, lo, hi }; }
    static Law poisson(double mean) { return { LAW_POISSON, mean, 0.0 }; }
    static Law gamma(double shape, double scale) { return { LAW_GAMMA, shape, scale }; }          // host/gamma_icdf.hpp; 0.01 <= shape <= 1000
    static Law exponential(double rate) { return { LAW_EXPONENTIAL, rate, 0.0 }; }
};
using LawChooser = std::function<Law(int timeIndex, int factor)>;

// the three factors of a Merton jump-diffusion: Brownian increment, standard normal jump size, Poisson jump count with mean λ·dt
inline LawChooser mertonLaws(const TimeDiscretization& td, double jumpIntensity) {
    return [td, jumpIntensity](int i, int f) { return f == 0 ? Law::normal(std::sqrt(td.getTimeStep(i))) : f == 1 ? Law::normal(1.0) : Law::poisson(jumpIntensity * td.getTimeStep(i)); };
}

// one factor: a gamma process, increment i ~ Gamma(shapePerTime · dt_i, scale) [unverified: finmath-lib's GammaProcess]
inline LawChooser gammaProcessLaws(const TimeDiscretization& td, double shapePerTime, double scale) {
    return [td, shapePerTime, scale](int i, int) { return Law::gamma(shapePerTime * td.getTimeStep(i), scale); };
}

// the two factors of a variance-gamma process: the gamma clock Γ_i ~ Gamma(dt_i/ν, ν) and a standard normal Z_i; the increment is
// θ·Γ_i + σ·sqrt(Γ_i)·Z_i (varianceGammaIncrement) [unverified: the layout is this project's, as the Merton layout is]
inline LawChooser varianceGammaLaws(const TimeDiscretization& td, double nu) {
    return [td, nu](int i, int f) { return f == 0 ? Law::gamma(td.getTimeStep(i) / nu, nu) : Law::normal(1.0); };
}

class IndependentIncrementsBase : public BrownianMotion {
public:
    IndependentIncrementsBase(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed, LawChooser laws)
        : td_(std::move(td)), factors_(numberOfFactors), paths_(numberOfPaths), seed_(seed), laws_(std::move(laws)) {}
    RV getBrownianIncrement(int timeIndex, int factor) const override {
        std::call_once(generated_, [this] { generate(); });
        return inc_.at((size_t)timeIndex * factors_ + factor);
    }
    const TimeDiscretization& getTimeDiscretization() const override { return td_; }
    int getNumberOfFactors() const override { return factors_; }
    int64_t getNumberOfPaths() const override { return paths_; }
    int getSeed() const { return seed_; }
protected:
    virtual void generate() const = 0;
    void lawArrays(std::vector<int32_t>& kind, std::vector<double>& a, std::vector<double>& b) const {
        const int steps = td_.getNumberOfTimeSteps();
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < factors_; ++f) { const Law law = laws_(i, f); kind.push_back(law.kind); a.push_back(law.a); b.push_back(law.b); }
    }
    TimeDiscretization td_;
    int factors_;
    int64_t paths_;
    int seed_;
    LawChooser laws_;
    mutable std::vector<RV> inc_;
    mutable std::once_flag generated_;
};

class IndependentIncrementsFromICDF final : public IndependentIncrementsBase {
public:
    IndependentIncrementsFromICDF(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed, LawChooser laws, const RandomVariableFactory* factory)
        : IndependentIncrementsBase(std::move(td), numberOfFactors, numberOfPaths, seed, std::move(laws)), factory_(factory) {}
    RV getRandomVariableForConstant(double value) const override { return factory_->createRandomVariable(value); }
private:
    void generate() const override {
        const int steps = td_.getNumberOfTimeSteps();
        std::vector<int32_t> kind; std::vector<double> a, b;
        lawArrays(kind, a, b);
        std::vector<double> all((size_t)steps * factors_ * (size_t)paths_);
        independentIncrements(seed_, steps, factors_, paths_, kind.data(), a.data(), b.data(), all.data());
        inc_.reserve((size_t)steps * factors_);
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < factors_; ++f) {
                const double* p = all.data() + ((size_t)i * factors_ + f) * (size_t)paths_;
                inc_.push_back(factory_->createRandomVariable(td_.getTime(i + 1), std::vector<double>(p, p + paths_)));
            }
    }
    const RandomVariableFactory* factory_;
};

class IndependentIncrementsFromICDFHip final : public IndependentIncrementsBase {
public:
    IndependentIncrementsFromICDFHip(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed, LawChooser laws, int64_t pathOffset = 0)
        : IndependentIncrementsBase(std::move(td), numberOfFactors, numberOfPaths, seed, std::move(laws)), offset_(pathOffset) {}
    RV getRandomVariableForConstant(double value) const override { return RandomVariableHip::of(-std::numeric_limits<double>::infinity(), value); }
private:
    void generate() const override {
        const int steps = td_.getNumberOfTimeSteps();
        std::vector<int32_t> kind; std::vector<double> a, b;
        lawArrays(kind, a, b);
        std::vector<fmhip_vec> h((size_t)steps * factors_);
        check(fmhip_increments_generate_device(seed_, steps, factors_, paths_, offset_, kind.data(), a.data(), b.data(), h.data()));
        inc_.reserve(h.size());
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < factors_; ++f)
                inc_.push_back(RandomVariableHip::of(td_.getTime(i + 1), DeviceVector(h[(size_t)i * factors_ + f]), paths_));
    }
    int64_t offset_;
};

// θ·Γ_i + σ·sqrt(Γ_i)·Z_i from increments laid out by varianceGammaLaws, in RandomVariable methods (the fusion front-end sees them)
inline RV varianceGammaIncrement(const BrownianMotion& increments, int timeIndex, double sigma, double theta) {
    const RV g = increments.getIncrement(timeIndex, 0), z = increments.getIncrement(timeIndex, 1);
    return g->mult(theta)->addProduct(g->sqrt()->mult(z), sigma);
}

} // namespace fmhost
