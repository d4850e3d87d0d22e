// sobol_brownian_motion.hpp — the quasi-Monte-Carlo Brownian motion in the C++ host mirror, beside independent_increments.hpp: Sobol'
// points through a Brownian bridge or increment by increment (host/sobol.hpp is the definition) — what finmath-lib's
// SobolSequence taken through BrownianMotionFromRandomNumberGenerator and BrownianBridge serve [unverified: finmath-lib is not vendored].
//   BrownianMotionFromSobolSequence      draws by the definition on the host and hands every increment to the injected factory: every
//                                        back end sees the same numbers
//   BrownianMotionFromSobolSequenceHip   the same numbers GENERATED ON THE DEVICE (fmhip_bm_generate_sobol_device), equal to the bit
// Both hold paths pathOffset … pathOffset + numberOfPaths of the whole motion.
#pragma once
#include <mutex>

#include "random_variable.hpp"
#include "sobol.hpp"

namespace fmhost {

class BrownianMotionFromSobolSequenceBase : public BrownianMotion {
public:
    BrownianMotionFromSobolSequenceBase(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed, int construction, bool randomize, int64_t pathOffset)
        : td_(std::move(td)), factors_(numberOfFactors), paths_(numberOfPaths), offset_(pathOffset), seed_(seed), construction_(construction), randomize_(randomize) {}
    RV getBrownianIncrement(int timeIndex, int factor) const override {
        std::call_once(generated_, [this] { generate(); });
        return inc_.at((size_t)timeIndex * factors_ + factor);
    }
    const TimeDiscretization& getTimeDiscretization() const override { return td_; }
    int getNumberOfFactors() const override { return factors_; }
    int64_t getNumberOfPaths() const override { return paths_; }
    int getSeed() const { return seed_; }
    int getConstruction() const { return construction_; }
protected:
    virtual void generate() const = 0;
    std::vector<double> timeSteps() const {
        std::vector<double> dt((size_t)td_.getNumberOfTimeSteps());
        for (size_t i = 0; i < dt.size(); ++i) dt[i] = td_.getTimeStep((int)i);
        return dt;
    }
    TimeDiscretization td_;
    int factors_;
    int64_t paths_, offset_;
    int seed_, construction_;
    bool randomize_;
    mutable std::vector<RV> inc_;
    mutable std::once_flag generated_;
};

class BrownianMotionFromSobolSequence final : public BrownianMotionFromSobolSequenceBase {
public:
    BrownianMotionFromSobolSequence(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed, const RandomVariableFactory* factory,
                                    int construction = FM_SOBOL_BRIDGE, bool randomize = true, int64_t pathOffset = 0)
        : BrownianMotionFromSobolSequenceBase(std::move(td), numberOfFactors, numberOfPaths, seed, construction, randomize, pathOffset), factory_(factory) {}
    RV getRandomVariableForConstant(double value) const override { return factory_->createRandomVariable(value); }
private:
    void generate() const override {
        const std::vector<double> dt = timeSteps();
        const int steps = (int)dt.size();
        std::vector<double> all((size_t)steps * factors_ * (size_t)paths_);
        sobolIncrements(seed_, randomize_ ? 1 : 0, construction_, steps, factors_, paths_, offset_, dt.data(), all.data());
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < factors_; ++f) {
                const double* first = all.data() + ((size_t)i * factors_ + f) * (size_t)paths_;
                inc_.push_back(factory_->createRandomVariable(td_.getTime(i + 1), std::vector<double>(first, first + paths_)));
            }
    }
    const RandomVariableFactory* factory_;
};

class BrownianMotionFromSobolSequenceHip final : public BrownianMotionFromSobolSequenceBase {
public:
    BrownianMotionFromSobolSequenceHip(TimeDiscretization td, int numberOfFactors, int64_t numberOfPaths, int seed,
                                       int construction = FM_SOBOL_BRIDGE, bool randomize = true, int64_t pathOffset = 0)
        : BrownianMotionFromSobolSequenceBase(std::move(td), numberOfFactors, numberOfPaths, seed, construction, randomize, pathOffset) {}
    RV getRandomVariableForConstant(double value) const override { return RandomVariableHip::of(-std::numeric_limits<double>::infinity(), value); }
private:
    void generate() const override {
        const std::vector<double> dt = timeSteps();
        const int steps = (int)dt.size();
        std::vector<fmhip_vec> h((size_t)steps * factors_);
        check(fmhip_bm_generate_sobol_device(seed_, randomize_ ? 1 : 0, construction_, steps, factors_, paths_, offset_, dt.data(), h.data()));
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < factors_; ++f)
                inc_.push_back(RandomVariableHip::of(td_.getTime(i + 1), DeviceVector(h[(size_t)i * factors_ + f]), paths_));
    }
};

} // namespace fmhost
