// test_regression.cpp — MonteCarloConditionalExpectationRegression of the C++ host mirror (host/regression.hpp: the normal equations from
// one fmhip_cross_moments call) against the CPU twin (fmhost::RandomVariableFromFloatArray: b_i.mult(b_j).getAverage() pair by pair)
// through the same interface; eager and fused; the mirror against itself with FMHIP_DEVICE_CROSS_MOMENTS=0; a deterministic basis
// function and a collinear one.  Basis 1, z, z², w of standard normals (condition number ≈ 9): the twin's fp32 products move a
// parameter by less than 1e-5.  Built and run by tests/test_gpu_cpp_regression.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../finmath-lib-cuda-extensions_amd/host/regression.hpp"
#include "../../oracle/host/random_variable_cpu.hpp"

using namespace fmhost;
static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } } while (0)

static std::vector<double> parameters(const RandomVariableFactory& f, const std::vector<double>& z, const std::vector<double>& w, const std::vector<double>& y, bool collinear, RV* ce = nullptr) {
    RV Z = f.createRandomVariable(0.0, z), W = f.createRandomVariable(0.0, w), Y = f.createRandomVariable(0.0, y);
    std::vector<RV> basis = { f.createRandomVariable(1.0), Z, Z->mult(Z), W };
    if (collinear) basis.push_back(f.createRandomVariable(-2.0));                   // a second constant
    MonteCarloConditionalExpectationRegression est(basis);
    if (ce) *ce = est.getConditionalExpectation(Y);
    return est.getLinearRegressionParameters(Y);
}

static void run(const RandomVariableFactory& hip, const RandomVariableFactory& cpu, const char* what) {
    std::mt19937_64 rng(2025);
    std::normal_distribution<double> normal;
    const int n = 100000;
    std::vector<double> z((size_t)n), w((size_t)n), y((size_t)n);
    for (int i = 0; i < n; ++i) { z[(size_t)i] = (double)(float)normal(rng); w[(size_t)i] = (double)(float)normal(rng); y[(size_t)i] = (double)(float)(1.0 + 0.5 * z[(size_t)i] - 0.25 * z[(size_t)i] * z[(size_t)i] + 0.3 * w[(size_t)i] + 0.1 * normal(rng)); }
    RV ceh, cec;
    const std::vector<double> bh = parameters(hip, z, w, y, false, &ceh), bc = parameters(cpu, z, w, y, false, &cec);
    const double want[4] = { 1.0, 0.5, -0.25, 0.3 };
    for (int i = 0; i < 4; ++i) { EXPECT(std::fabs(bh[(size_t)i] - bc[(size_t)i]) <= 1e-5, what); EXPECT(std::fabs(bh[(size_t)i] - want[i]) <= 0.01, what); }
    const std::vector<double> vh = ceh->getRealizations(), vc = cec->getRealizations();
    double worst = 0.0; for (int i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs(vh[(size_t)i] - vc[(size_t)i]));
    EXPECT(worst <= 1e-4, what);
    const std::vector<double> dh = parameters(hip, z, w, y, true);
    // two constants: the larger one (diagonal 4 against 1) is the earlier pivot, the other is dropped, and it carries the intercept
    EXPECT(dh.size() == 5 && dh[0] == 0.0 && std::fabs(-2.0 * dh[4] - bh[0]) <= 1e-5, what);
}

int main() {
    // the solver on a fixed matrix and on a singular one
    {
        const std::vector<double> A = { 24, 16, 20, 16, 14, 12, 20, 12, 30 }, b = { 1, 2, 3 };
        const std::vector<double> x = solveNormalEquations(A, b, 3);
        for (int i = 0; i < 3; ++i) { double r = -b[(size_t)i]; for (int j = 0; j < 3; ++j) r += A[(size_t)i * 3 + j] * x[(size_t)j]; EXPECT(std::fabs(r) <= 1e-12, "solver residual"); }
        const std::vector<double> S = { 1, 1, 0, 1, 1, 0, 0, 0, 0 }, c = { 2, 2, 0 };
        const std::vector<double> s = solveNormalEquations(S, c, 3);
        EXPECT(s[0] == 2.0 && s[1] == 0.0 && s[2] == 0.0, "pivot rule");
    }
    check(fmhip_init(-1));
    RandomVariableHipFactory hip;
    RandomVariableFloatFactory cpu;
    for (int fused = 0; fused < 2; ++fused) {
        check(fmhip_set_fusion(fused, nullptr));
        run(hip, cpu, fused ? "one-pass regression vs cpu twin (fused)" : "one-pass regression vs cpu twin (eager)");
        setenv("FMHIP_DEVICE_CROSS_MOMENTS", "0", 1);
        run(hip, cpu, "pair by pair (FMHIP_DEVICE_CROSS_MOMENTS=0) vs cpu twin");
        unsetenv("FMHIP_DEVICE_CROSS_MOMENTS");
    }
    check(fmhip_shutdown());
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
