// test_levy_increments.cpp — the gamma and the exponential law in host/increments.hpp and in the C++ mirror (host/independent_increments.hpp).
//   test_levy_increments cpu      no device: equal shapes share one entry of constants, which lie beside the Poisson tables; the draws by
//                                 hand from the first MT19937 doubles; the argument errors; kind 3 is still no law; the mirror over the CPU twin
//   test_levy_increments device   IndependentIncrementsFromICDFHip (generated on the device) against IndependentIncrementsFromICDF over the
//                                 device factory (drawn on the host, uploaded): gamma and exponential draws EQUAL, every one; a block behind
//                                 a path offset; a variance-gamma path written against the RandomVariable interface on both
// Built and run by tests/test_gamma_icdf_cpu.py and tests/test_gpu_cpp_levy_increments.py.
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

static bool rejected(const std::vector<int32_t>& k, const std::vector<double>& a, const std::vector<double>& b) {
    try { checkedIncrementLaws(1, (int)k.size(), 10, 0, k.data(), a.data(), b.data()); } catch (const std::invalid_argument& e) { return std::strstr(e.what(), "(step 0, factor ") != nullptr; }
    return false;
}

static void definition() {
    const std::vector<int32_t> k = { LAW_GAMMA, LAW_POISSON, LAW_GAMMA, LAW_GAMMA, LAW_EXPONENTIAL, LAW_NORMAL };
    const std::vector<double> a = { 0.06, 1.0, 2.5, 0.06, 3.0, 1.0 }, b = { 0.2, 9.0, 1.0, 7.0, 9.0, 9.0 };
    const IncrementLaws L = checkedIncrementLaws(2, 3, 10, 0, k.data(), a.data(), b.data());
    EXPECT(L.laws[0].table_len == (uint32_t)FM_GAMMA_CONSTS && L.laws[0].table_offset == 0, "a shape's constants are an entry of the table block");
    EXPECT(L.laws[3].table_offset == L.laws[0].table_offset && L.laws[3].table_len == L.laws[0].table_len, "equal shapes share one entry, whatever the scale");
    EXPECT(L.laws[1].table_offset == (uint32_t)FM_GAMMA_CONSTS && L.laws[2].table_offset == L.laws[1].table_offset + L.laws[1].table_len, "entries lie one behind the other, Poisson tables among them");
    EXPECT(L.tables.size() == (size_t)L.laws[2].table_offset + FM_GAMMA_CONSTS && L.laws[4].table_len == 0 && L.laws[5].table_len == 0 && L.laws[4].b == 0.0, "nothing else is in the table block");
    int sign = 0;
    EXPECT(L.tables[FM_GC_LGAMMA] == ::lgamma_r(0.06, &sign) && L.tables[FM_GC_INV_SHAPE] == 1.0 / 0.06 && L.tables[L.laws[2].table_offset + FM_GC_LGAMMA1] == ::lgamma_r(3.5, &sign), "the constants");
    static_assert(sizeof(IncrementLaws::Law) == 32, "the descriptor keeps its size");
    // the draws by hand
    MT19937 mt((int64_t)31415);
    std::vector<double> out(6 * 2);
    independentIncrements(31415, 2, 3, 2, k.data(), a.data(), b.data(), out.data());
    for (int path = 0; path < 2; ++path)
        for (size_t s = 0; s < 6; ++s) {
            const double u = mt.nextDouble(), got = out[s * 2 + (size_t)path];
            double want;
            if (k[s] == LAW_GAMMA) want = fm_inverse_gamma_cdf(a[s], gammaConsts(a[s]).data(), u) * b[s];
            else if (k[s] == LAW_EXPONENTIAL) want = (0.0 - fm_log64(1.0 - u)) / a[s];
            else if (k[s] == LAW_NORMAL) want = inverseNormalCdf(u) * a[s];
            else { const std::vector<double> F = poissonTable(a[s]); want = poissonFromTable(F.data(), (int)F.size(), u); }
            EXPECT(std::memcmp(&got, &want, 8) == 0, "a draw is its law's inverse CDF of the uniform of its place in the stream");
        }
    const double nan = std::nan(""), inf = HUGE_VAL;
    EXPECT(rejected({ 3 }, { 1.0 }, { 0.0 }) && rejected({ 6 }, { 1.0 }, { 1.0 }), "kind 3 is no law, nor is 6");
    for (double shape : { 0.0, -1.0, nan, inf, 0.00999, 1000.001 }) EXPECT(rejected({ LAW_GAMMA }, { shape }, { 1.0 }), "a shape outside the caps");
    for (double scale : { 0.0, -1.0, nan, inf }) EXPECT(rejected({ LAW_GAMMA }, { 1.0 }, { scale }), "a scale that is not positive and finite");
    for (double rate : { 0.0, -1.0, nan, inf }) EXPECT(rejected({ LAW_EXPONENTIAL }, { rate }, { 0.0 }), "a rate that is not positive and finite");
    EXPECT(!rejected({ LAW_GAMMA, LAW_GAMMA, LAW_EXPONENTIAL }, { FM_GAMMA_SHAPE_MIN, FM_GAMMA_SHAPE_MAX, 1e-300 }, { 1e-300, 1e300, 0.0 }), "the caps themselves are inside");
    std::vector<int32_t> km(10923, LAW_GAMMA); std::vector<double> am, bm(10923, 1.0);
    for (int i = 0; i < 10923; ++i) am.push_back(1.0 + 1e-4 * i);
    bool threw = false;
    try { checkedIncrementLaws(10923, 1, 1, 0, km.data(), am.data(), bm.data()); } catch (const std::invalid_argument& e) { threw = std::strstr(e.what(), "step 10922") != nullptr; }
    EXPECT(threw, "more constants than the 2^16 table doubles");
}

static std::vector<double> varianceGammaPath(const BrownianMotion& inc, int steps) {
    RV x = inc.getRandomVariableForConstant(std::log(100.0));
    for (int i = 0; i < steps; ++i) x = x->add(0.003)->add(varianceGammaIncrement(inc, i, 0.2, -0.14));
    return x->exp()->getRealizations();
}

static void mirrorOnTheTwin() {
    RandomVariableFloatFactory cpu;
    const TimeDiscretization td(0.0, 4, 0.25);
    IndependentIncrementsFromICDF g(td, 1, 20000, 4711, gammaProcessLaws(td, 5.0, 0.2), &cpu);
    double mean = 0.0;
    for (double v : g.getIncrement(2, 0)->getRealizations()) { mean += v; EXPECT(v >= 0.0, "gamma increments are not negative"); }
    EXPECT(std::fabs(mean / 20000.0 - 0.25) < 4 * std::sqrt(0.05 / 20000.0), "their mean is shape * scale");
    IndependentIncrementsFromICDF vg(td, 2, 20000, 4711, varianceGammaLaws(td, 0.2), &cpu);
    EXPECT(vg.getIncrement(2, 0)->getFiltrationTime() == 0.75 && vg.getNumberOfFactors() == 2, "the increments carry t_{i+1}");
    const std::vector<double> s = varianceGammaPath(vg, 4);
    double avg = 0.0; for (double v : s) avg += v;
    EXPECT(avg / 20000.0 > 80.0 && avg / 20000.0 < 120.0, "a variance-gamma path stays where it should");
    IndependentIncrementsFromICDF e(td, 1, 20000, 1, [](int, int) { return Law::exponential(4.0); }, &cpu);
    mean = 0.0; for (double v : e.getIncrement(0, 0)->getRealizations()) mean += v;
    EXPECT(std::fabs(mean / 20000.0 - 0.25) < 4 * 0.25 / std::sqrt(20000.0), "the mean of an exponential law is 1 / rate");
}

static void device() {
    check(fmhip_init(0));
    {
        RandomVariableHipFactory hip;
        const TimeDiscretization td(0.0, 5, 0.25);
        const int64_t n = 200003;
        const LawChooser laws = [td](int i, int f) { return f == 0 ? Law::gamma(td.getTimeStep(i) / 0.2, 0.2) : f == 1 ? Law::normal(1.0) : f == 2 ? Law::exponential(1.0 + i) : Law::gamma(0.01 + 200.0 * i, 3.0); };
        IndependentIncrementsFromICDF host(td, 4, n, 4711, laws, &hip);
        IndependentIncrementsFromICDFHip dev(td, 4, n, 4711, laws);
        IndependentIncrementsFromICDFHip part(td, 4, 1000, 4711, laws, 150001);
        int64_t off_by_one_ulp = 0;
        for (int i = 0; i < 5; ++i)
            for (int f = 0; f < 4; ++f) {
                const std::vector<double> h = host.getIncrement(i, f)->getRealizations(), d = dev.getIncrement(i, f)->getRealizations(), p = part.getIncrement(i, f)->getRealizations();
                EXPECT(h.size() == (size_t)n && d.size() == (size_t)n && p.size() == 1000, "sizes");
                for (size_t k = 0; k < (size_t)n; ++k)
                    if (h[k] != d[k]) {
                        const bool tail = f == 1 && std::fabs(h[k]) > 1.4395 && (float)d[k] == std::nextafterf((float)h[k], (float)d[k] > (float)h[k] ? HUGE_VALF : -HUGE_VALF);
                        EXPECT(tail, "gamma and exponential draws are equal; only a normal tail draw may differ, by one fp32 ulp");
                        ++off_by_one_ulp;
                    }
                for (size_t k = 0; k < 1000; ++k) EXPECT(p[k] == d[150001 + k], "a block behind a path offset is a slice of the whole");
                EXPECT(dev.getIncrement(i, f)->getFiltrationTime() == td.getTime(i + 1), "filtration time");
            }
        EXPECT(off_by_one_ulp <= 2, "a handful in 10^8");
        if (off_by_one_ulp == 0) {
            const std::vector<double> a = varianceGammaPath(host, 5), b = varianceGammaPath(dev, 5);
            EXPECT(a == b, "a variance-gamma path on host-drawn and on device-generated increments");
        }
        std::printf("%lld of %lld draws one ulp off\n", (long long)off_by_one_ulp, (long long)(20 * n));
    }
    check(fmhip_shutdown());
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "cpu";
    if (mode == "device") device();
    else { definition(); mirrorOnTheTwin(); }
    if (failures) { std::printf("%d FAILURES\n", failures); return 1; }
    std::printf("OK %s\n", mode.c_str());
    return 0;
}
