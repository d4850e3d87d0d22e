// test_increments.cpp — host/increments.hpp (the definition of increments with a law per time step and factor) and the C++ mirror's
// IndependentIncrementsFromICDF (host/independent_increments.hpp).
//   test_increments cpu      no device: the Poisson tables (first entry exp(−mean) to the bit, rising, ending in 1.0, under 300 entries at
//                            the cap), draws one ulp either side of a table entry, mean 0, equal means sharing a table, uniform known
//                            answers against the first MT19937 doubles, all-normal laws against mersenneIncrements bit for bit, every
//                            argument error, and the mirror class over the CPU twin's factory
//   test_increments device   on the device: IndependentIncrementsFromICDFHip (generated on the device) against IndependentIncrementsFromICDF
//                            over the device factory (drawn on the host, uploaded) — Poisson and normal-central draws equal — whole and as
//                            a block behind a path offset, and a Merton step written against the RandomVariable interface on both
// Built and run by tests/test_increments_cpu.py and tests/test_gpu_cpp_increments.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../finmath-lib-cuda-extensions_amd/host/independent_increments.hpp"
#include "../../oracle/host/random_variable_cpu.hpp"

using namespace fmhost;
static int failures = 0;
#define EXPECT(cond, what) do { if (!(cond)) { std::printf("FAIL %s (%s:%d)\n", what, __FILE__, __LINE__); ++failures; } } while (0)

static bool rejected(int steps, int factors, int64_t paths, int64_t offset, const std::vector<int32_t>& k, const std::vector<double>& a, const std::vector<double>& b) {
    try { checkedIncrementLaws(steps, factors, paths, offset, k.data(), a.data(), b.data()); } catch (const std::invalid_argument& e) { return std::strlen(e.what()) > 0; }
    return false;
}

static void tables() {
    for (double mean : { 0.02, 0.5, 1.0, 2.5, 30.0, 100.0, 127.99, 128.0 }) {
        const std::vector<double> F = poissonTable(mean);
        const double first = std::exp(-mean);
        EXPECT(std::memcmp(&F[0], &first, 8) == 0, "F[0] is exp(-mean) to the bit");
        EXPECT(F.back() == 1.0 && F.size() < 300 && F.size() > (size_t)mean, "a table ends in 1.0, past the mode, under 300 entries");
        for (size_t k = 1; k < F.size(); ++k) EXPECT(F[k] >= F[k - 1], "a table rises");
        for (size_t k = 1; k + 1 < F.size(); ++k) EXPECT(F[k] > F[k - 1], "it rises strictly before its last entry");
        // by hand: the recurrence in the order of the definition
        double p = first, sum = first;
        for (size_t k = 1; k + 1 < F.size(); ++k) { p = p * mean / (double)k; sum = sum + p; EXPECT(sum == F[k], "the recurrence p = p * mean / k, F[k] = F[k-1] + p"); }
        // a uniform one ulp either side of an entry
        for (size_t k = 0; k + 1 < F.size(); k += (F.size() > 40 ? 17 : 1)) {
            EXPECT(poissonFromTable(F.data(), (int)F.size(), F[k]) == (int)k, "u == F[k] gives k");
            EXPECT(poissonFromTable(F.data(), (int)F.size(), std::nextafter(F[k], 0.0)) == (int)k - (k > 0 && !(F[k - 1] < std::nextafter(F[k], 0.0)) ? 1 : 0), "one ulp below F[k] gives k");
            EXPECT(poissonFromTable(F.data(), (int)F.size(), std::nextafter(F[k], 2.0)) == (int)k + 1, "one ulp above F[k] gives k + 1");
        }
        EXPECT(poissonFromTable(F.data(), (int)F.size(), 0.0) == 0 && poissonFromTable(F.data(), (int)F.size(), 1.0 - 0x1.0p-53) == (int)F.size() - 1, "u = 0 and the largest u");
    }
    const std::vector<double> one = poissonTable(1.0);
    EXPECT(poissonFromTable(one.data(), (int)one.size(), std::nextafter(std::exp(-1.0), 0.0)) == 0 && poissonFromTable(one.data(), (int)one.size(), std::nextafter(std::exp(-1.0), 1.0)) == 1, "mean 1: one ulp either side of F[0] gives 0 / 1");
    const std::vector<double> zero = poissonTable(0.0);
    EXPECT(zero.size() == 1 && zero[0] == 1.0, "mean 0 is the table {1.0}");
    // equal means share a table, −0 is 0
    const std::vector<int32_t> k = { LAW_POISSON, LAW_NORMAL, LAW_POISSON, LAW_POISSON, LAW_UNIFORM, LAW_POISSON };
    const std::vector<double> a = { 0.5, 1.0, 3.0, 0.5, -1.0, -0.0 }, b = { 9.0, 9.0, 9.0, 9.0, 3.0, 9.0 };
    const IncrementLaws L = checkedIncrementLaws(2, 3, 10, 0, k.data(), a.data(), b.data());
    EXPECT(L.laws[0].table_offset == 0 && L.laws[3].table_offset == 0 && L.laws[3].table_len == L.laws[0].table_len, "equal means share a table");
    EXPECT(L.laws[2].table_offset == L.laws[0].table_len && L.laws[5].table_offset == L.laws[2].table_offset + L.laws[2].table_len && L.laws[5].table_len == 1, "tables lie one behind the other");
    EXPECT(L.tables.size() == (size_t)L.laws[5].table_offset + 1 && L.laws[1].table_len == 0 && L.laws[4].table_len == 0, "nothing else is in the table block");
}

static void definition() {
    // uniform known answers against the first MT19937 doubles
    MT19937 mt((int64_t)31415);
    std::vector<double> u(6); for (double& v : u) v = mt.nextDouble();
    const std::vector<int32_t> k = { LAW_UNIFORM, LAW_UNIFORM, LAW_UNIFORM };
    const std::vector<double> a = { 0.0, -1.0, 2.0 }, b = { 1.0, 3.0, 2.0 };
    std::vector<double> out(6);
    independentIncrements(31415, 3, 1, 2, k.data(), a.data(), b.data(), out.data());
    for (int path = 0; path < 2; ++path) {
        EXPECT(out[(size_t)(0 * 2 + path)] == u[(size_t)(path * 3)], "uniform on [0, 1) is nextDouble itself");
        EXPECT(out[(size_t)(1 * 2 + path)] == -1.0 + 4.0 * u[(size_t)(path * 3 + 1)], "uniform on [-1, 3)");
        EXPECT(out[(size_t)(2 * 2 + path)] == 2.0, "a degenerate uniform");
    }
    // all-normal laws are mersenneIncrements
    const std::vector<double> dt = { 0.25, 0.0, 1.5, 0.1 };
    for (int seed : { 3141, 0, -1 }) {
        const int steps = 4, factors = 3; const int64_t n = 2000;
        std::vector<int32_t> kn((size_t)steps * factors, LAW_NORMAL); std::vector<double> an, bn((size_t)steps * factors, 0.0);
        for (int i = 0; i < steps; ++i) for (int f = 0; f < factors; ++f) an.push_back(std::sqrt(dt[(size_t)i]));
        std::vector<double> want((size_t)steps * factors * n), got(want.size());
        mersenneIncrements(seed, steps, factors, n, dt.data(), want.data());
        independentIncrements(seed, steps, factors, n, kn.data(), an.data(), bn.data(), got.data());
        EXPECT(std::memcmp(want.data(), got.data(), 8 * want.size()) == 0, "all-normal laws equal mersenneIncrements bit for bit");
    }
    // the argument errors
    const double nan = std::nan(""), inf = HUGE_VAL;
    EXPECT(rejected(1, 1, 10, 0, { 3 }, { 1.0 }, { 0.0 }) && rejected(1, 1, 10, 0, { -1 }, { 1.0 }, { 0.0 }), "unknown kind");
    EXPECT(rejected(1, 1, 10, 0, { LAW_NORMAL }, { -1.0 }, { 0.0 }) && rejected(1, 1, 10, 0, { LAW_NORMAL }, { nan }, { 0.0 }), "negative or NaN scale");
    EXPECT(rejected(1, 1, 10, 0, { LAW_POISSON }, { -1.0 }, { 0.0 }) && rejected(1, 1, 10, 0, { LAW_POISSON }, { nan }, { 0.0 }) && rejected(1, 1, 10, 0, { LAW_POISSON }, { 128.5 }, { 0.0 }), "negative, NaN or too large a mean");
    EXPECT(rejected(1, 1, 10, 0, { LAW_UNIFORM }, { 2.0 }, { 1.0 }) && rejected(1, 1, 10, 0, { LAW_UNIFORM }, { 0.0 }, { inf }) && rejected(1, 1, 10, 0, { LAW_UNIFORM }, { nan }, { 1.0 }), "a > b, non-finite bounds");
    EXPECT(rejected(0, 1, 10, 0, { 0 }, { 1.0 }, { 0.0 }) && rejected(1, 0, 10, 0, { 0 }, { 1.0 }, { 0.0 }) && rejected(1, 1, -1, 0, { 0 }, { 1.0 }, { 0.0 }) && rejected(1, 1, 1, -1, { 0 }, { 1.0 }, { 0.0 }), "counts");
    EXPECT(rejected(1 << 20, 1 << 5, 1, 0, { 0 }, { 1.0 }, { 0.0 }), "more than 2^24 laws");
    EXPECT(rejected(1, 1, 10, (int64_t(1) << 43), { 0 }, { 1.0 }, { 0.0 }) && !rejected(1, 1, 10, (int64_t(1) << 43) - 10, { 0 }, { 1.0 }, { 0.0 }), "the 2^44-word limit");
    std::vector<int32_t> km(400, LAW_POISSON); std::vector<double> am, bm(400, 0.0);
    for (int i = 0; i < 400; ++i) am.push_back(100.0 + 1e-3 * i);
    EXPECT(rejected(400, 1, 10, 0, km, am, bm), "more than 2^16 table doubles");
    EXPECT(!rejected(400, 1, 10, 0, km, std::vector<double>(400, 100.0), bm), "one table, however many laws name it");
}

static std::vector<double> mertonStep(const BrownianMotion& inc, int steps) {          // a Merton log-Euler path, RandomVariable methods only
    RV x = inc.getRandomVariableForConstant(std::log(100.0));
    for (int i = 0; i < steps; ++i) {
        RV dw = inc.getIncrement(i, 0), z = inc.getIncrement(i, 1), dn = inc.getIncrement(i, 2);
        x = x->add(-0.01)->addProduct(dw, 0.2)->addProduct(dn, -0.1)->addProduct(dn->sqrt()->mult(z), 0.15);
    }
    return x->exp()->getRealizations();
}

static void mirrorOnTheTwin() {
    RandomVariableFloatFactory cpu;
    const TimeDiscretization td(0.0, 4, 0.25);
    IndependentIncrementsFromICDF inc(td, 3, 5000, 4711, mertonLaws(td, 2.0), &cpu);
    EXPECT(inc.getIncrement(2, 1)->getFiltrationTime() == 0.75 && inc.getNumberOfFactors() == 3 && inc.getNumberOfPaths() == 5000, "the increments carry t_{i+1}");
    const std::vector<double> n = inc.getIncrement(1, 2)->getRealizations();
    double mean = 0.0; for (double v : n) { mean += v; EXPECT(v == std::floor(v) && v >= 0.0, "jump counts are whole numbers"); }
    EXPECT(std::fabs(mean / 5000.0 - 0.5) < 0.05, "their mean is lambda * dt");
    const std::vector<double> s = mertonStep(inc, 4);
    double avg = 0.0; for (double v : s) avg += v;
    EXPECT(avg / 5000.0 > 60.0 && avg / 5000.0 < 110.0, "a Merton path stays where it should");
}

static void device() {
    check(fmhip_init(0));
    {
        RandomVariableHipFactory hip;
        const TimeDiscretization td(0.0, 5, 0.25);
        const int64_t n = 200003;
        IndependentIncrementsFromICDF host(td, 3, n, 4711, mertonLaws(td, 2.0), &hip);
        IndependentIncrementsFromICDFHip dev(td, 3, n, 4711, mertonLaws(td, 2.0));
        IndependentIncrementsFromICDFHip part(td, 3, 1000, 4711, mertonLaws(td, 2.0), 150001);
        int64_t off_by_one_ulp = 0;
        for (int i = 0; i < 5; ++i)
            for (int f = 0; f < 3; ++f) {
                const std::vector<double> h = host.getIncrement(i, f)->getRealizations(), d = dev.getIncrement(i, f)->getRealizations(), p = part.getIncrement(i, f)->getRealizations();
                EXPECT(h.size() == (size_t)n && d.size() == (size_t)n && p.size() == 1000, "sizes");
                const double scale = f == 0 ? 0.5 : 1.0;
                for (size_t k = 0; k < (size_t)n; ++k)
                    if (h[k] != d[k]) {
                        const bool tail = f < 2 && std::fabs(h[k]) / scale > 1.4395 && (float)d[k] == std::nextafterf((float)h[k], (float)d[k] > (float)h[k] ? HUGE_VALF : -HUGE_VALF);
                        EXPECT(tail, "only a normal tail draw may differ, by one fp32 ulp");
                        ++off_by_one_ulp;
                    }
                for (size_t k = 0; k < 1000; ++k) EXPECT(p[k] == d[150001 + k], "a block behind a path offset is a slice of the whole");
                EXPECT(dev.getIncrement(i, f)->getFiltrationTime() == td.getTime(i + 1), "filtration time");
            }
        EXPECT(off_by_one_ulp <= 2, "a handful in 10^8");
        if (off_by_one_ulp == 0) {
            const std::vector<double> a = mertonStep(host, 5), b = mertonStep(dev, 5);
            EXPECT(a == b, "a Merton path on host-drawn and on device-generated increments");
        }
        std::printf("%lld of %lld draws one ulp off\n", (long long)off_by_one_ulp, (long long)(15 * n));
    }
    check(fmhip_shutdown());
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "device") device();
    else { tables(); definition(); mirrorOnTheTwin(); }
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("OK %s\n", mode.c_str());
    return 0;
}
