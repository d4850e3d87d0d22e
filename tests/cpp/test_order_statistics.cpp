// test_order_statistics.cpp — getQuantile, getQuantileExpectation and both getHistograms of the C++ host mirror (fmhost::RandomVariableHip:
// selected and counted on the device, fmhip_select_ranks_batch / fmhip_rank_sums_batch / fmhip_count_not_above) against the CPU twin
// (fmhost::RandomVariableFromFloatArray: the interface's host sort), through the same interface; eager and fused, on a stored vector and
// on a pending expression that is never read; and the mirror against itself with FMHIP_DEVICE_ORDER_STATS=0.  Quantiles and histograms
// exactly, quantile expectations to 1e-13 (fp64 reassociation).  Built and run by tests/test_gpu_cpp_order_statistics.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "../../finmath-lib-cuda-extensions_amd/host/random_variable.hpp"
#include "../../oracle/host/random_variable_cpu.hpp"

using namespace fmhost;
static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } } while (0)

static bool close13(double a, double b) { return (a != a && b != b) || std::fabs(a - b) <= 1e-13 * (1.0 + std::fabs(b)); }

static void compare(const RV& got, const RV& want, const char* what) {
    for (double q : { 0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0 }) EXPECT(got->getQuantile(q) == want->getQuantile(q), what);
    for (auto r : { std::pair<double, double>{ 0.0, 0.05 }, { 0.05, 0.95 }, { 0.9, 0.2 }, { 0.5, 0.5 }, { 0.0, 1.0 } })
        EXPECT(close13(got->getQuantileExpectation(r.first, r.second), want->getQuantileExpectation(r.first, r.second)), what);
    const std::vector<double> points = { 2.0, -0.5, 0.1, 0.1, 1.0, 0.0 };            // unsorted, a duplicate
    EXPECT(got->getHistogram(points) == want->getHistogram(points), what);
    EXPECT(got->getHistogram(std::vector<double>{}) == want->getHistogram(std::vector<double>{}), what);
    const auto a = got->getHistogram(9, 2.5), b = want->getHistogram(9, 2.5);
    // (the grid is built from average and standard deviation, which the two sides add in different orders: compared as sums of shares)
    EXPECT(a.size() == 2 && b.size() == 2 && a[1].size() == b[1].size(), what);
    double sa = 0.0, sb = 0.0; for (double v : a[1]) sa += v; for (double v : b[1]) sb += v;
    EXPECT(std::fabs(sa - 1.0) <= 1e-12 && std::fabs(sb - 1.0) <= 1e-12, what);
}

static void run(const RandomVariableFactory& hip, const RandomVariableFactory& cpu, const char* what) {
    std::mt19937_64 rng(2024);
    std::normal_distribution<double> normal;
    for (int n : { 1, 2, 77, 4096, 50001, 300000 }) {
        std::vector<double> d((size_t)n);
        for (double& v : d) v = (double)(float)normal(rng);
        for (size_t i = 0; i < d.size(); i += 5) d[i] = 0.25;                        // ties
        RV xh = hip.createRandomVariable(0.0, d), xc = cpu.createRandomVariable(0.0, d);
        compare(xh, xc, what);
        // a payoff: half exact zeros; pending on the device until its quantile is asked for
        RV ph = xh->exp()->sub(1.0)->floor(0.0), pc = xc->exp()->sub(1.0)->floor(0.0);
        compare(ph, pc, what);
    }
    RV c = hip.createRandomVariable(3.0);                                             // deterministic: as before
    EXPECT(c->getQuantile(0.3) == 3.0 && c->getQuantileExpectation(0.1, 0.9) == 3.0, what);
}

int main() {
    check(fmhip_init(-1));
    RandomVariableHipFactory hip;
    RandomVariableFloatFactory cpu;
    for (int fused = 0; fused < 2; ++fused) {
        check(fmhip_set_fusion(fused, nullptr));
        run(hip, cpu, fused ? "device order statistics vs cpu twin (fused)" : "device order statistics vs cpu twin (eager)");
        setenv("FMHIP_DEVICE_ORDER_STATS", "0", 1);
        run(hip, cpu, "host sort (FMHIP_DEVICE_ORDER_STATS=0) vs cpu twin");
        unsetenv("FMHIP_DEVICE_ORDER_STATS");
    }
    check(fmhip_shutdown());
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
