// test_gamma_icdf.cpp — host/gamma_icdf.hpp where it can be seen: the header itself, compiled as host C++ (tests/test_gamma_icdf_cpu.py
// builds this with -ffp-contract=off and holds its output against references of its own).
//   exp | log     a hex double per line on stdin → fm_exp64 / fm_log64 of it, as a hex double
//   icdf          "shape u" per line (hex doubles) → fm_inverse_gamma_cdf(shape, gammaConsts(shape), u) and the Halley steps it took
//   p             "shape x" per line → fm_gamma_p
//   identities    the checks that need no reference; prints "OK identities"
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/host/increments.hpp"

using namespace fmhost;

#define CHECK(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(1); } } while (0)

// the steps fm_inverse_gamma_cdf takes: the same loop, counted (kept in step with the header by the comparison of its result below)
static int halley_steps(double shape, const double* consts, double u, double* result) {
    double x = fm_exp64((fm_log64(u) + consts[FM_GC_LGAMMA1]) * consts[FM_GC_INV_SHAPE]);
    const double q = 1.0 - u;
    if (shape > 1.0) {
        const double w = consts[FM_GC_WH_CENTRE] + fm_normal_quantile(u) * consts[FM_GC_WH_SLOPE];
        const double wh = shape * (w * w * w);
        if (w > 0.0 && wh > x) x = wh;
    } else if (u >= consts[FM_GC_SPLIT]) x = 1.0 - fm_log64(q / (1.0 - consts[FM_GC_SPLIT]));
    int steps = 0;
    if (x > 0.0)
        for (; steps < FM_GAMMA_HALLEY_CAP;) {
            const FmGammaTail tail = fm_gamma_tail(shape, consts[FM_GC_LGAMMA], x);
            const double error = x < shape + 1.0 ? tail.direct - u : q - tail.direct;
            const double density = tail.front / x;
            if (!(density > 0.0) || !(density < 0x1.0p1023)) break;
            ++steps;
            const double newton = error / density;
            double curvature = newton * ((shape - 1.0) / x - 1.0);
            if (curvature > 1.0) curvature = 1.0;
            const double move = newton / (1.0 - 0.5 * curvature);
            double next = x - move;
            if (!(next > 0.0)) next = 0.5 * x;
            const bool settled = std::fabs(move) <= 0x1.0p-30 * next;
            x = next;
            if (settled) break;
        }
    else x = 0.0;
    *result = x;
    return steps;
}

static void identities() {
    const double shapes[] = { 0.01, 0.0625, 0.5, 1.0, 2.5, 30.0, 1000.0 };
    // u = 0 → +0.0, for every shape and for the exponential law
    for (double shape : shapes) {
        const std::vector<double> c = gammaConsts(shape);
        const double x = fm_inverse_gamma_cdf(shape, c.data(), 0.0);
        CHECK(x == 0.0 && !std::signbit(x), "shape %g: u = 0 gives %a", shape, x);
    }
    { const double x = fm_exponential_icdf(2.0, 0.0); CHECK(x == 0.0 && !std::signbit(x), "exponential: u = 0 gives %a", x); }
    // monotone in u over 10^5 sorted draws per shape, and never beyond the cap of steps
    for (double shape : shapes) {
        const std::vector<double> c = gammaConsts(shape);
        MT19937 mt((int64_t)4711);
        std::vector<double> u(100000);
        for (double& v : u) v = mt.nextDouble();
        std::sort(u.begin(), u.end());
        double last = 0.0; int most = 0;
        for (double v : u) {
            double again;
            const int steps = halley_steps(shape, c.data(), v, &again);
            const double x = fm_inverse_gamma_cdf(shape, c.data(), v);
            CHECK(x == again || (x != x && again != again), "shape %g u %a: the counted loop is not the header's", shape, v);
            CHECK(x >= last, "shape %g: not monotone at u = %a: %a after %a", shape, v, x, last);
            CHECK(steps < FM_GAMMA_HALLEY_CAP, "shape %g u %a: the iteration ran into its cap", shape, v);
            if (steps > most) most = steps;
            last = x;
        }
        std::printf("shape %g: monotone over %zu draws, at most %d Halley steps\n", shape, u.size(), most);
    }
    // shape 1 is the exponential law with rate 1: to the last bit of the fp32 narrowing; in fp64 a few ulp apart at most
    {
        const std::vector<double> c = gammaConsts(1.0);
        MT19937 mt((int64_t)31415);
        double worst = 0.0;
        for (int i = 0; i < 100000; ++i) {
            const double u = mt.nextDouble();
            const double g = fm_inverse_gamma_cdf(1.0, c.data(), u), e = fm_exponential_icdf(1.0, u);
            const float gf = (float)g, ef = (float)e;
            CHECK(std::memcmp(&gf, &ef, 4) == 0, "u %a: gamma(1) %a, exponential %a", u, g, e);
            if (e > 0.0 && std::fabs(g - e) / e > worst) worst = std::fabs(g - e) / e;
        }
        CHECK(worst <= 0x1.0p-40, "gamma(1) against the exponential law: %g", worst);
        std::printf("shape 1 against the exponential law: largest relative difference %.3g\n", worst);
    }
    // shape 1/2 is half the square of a normal variable: x = inverseNormalCdf((1 + u)/2)² / 2
    {
        const std::vector<double> c = gammaConsts(0.5);
        MT19937 mt((int64_t)2718);
        double worst = 0.0;
        for (int i = 0; i < 100000; ++i) {
            const double u = mt.nextDouble();
            if (u > 1.0 - 0x1.0p-20) continue;                              // (1 + u)/2 rounds there: the identity's own argument loses its bits
            const double z = inverseNormalCdf(0.5 + 0.5 * u);
            const double want = 0.5 * z * z, got = fm_inverse_gamma_cdf(0.5, c.data(), u);
            if (want >= 0x1.0p-126) {
                // AS 241 has a relative accuracy of about 1e-16 in z; 0.5 + 0.5 u is exact but z near 0 carries the rounding of u/2 − 0 … none:
                // the bound is the issue's, 2^-40
                const double rel = std::fabs(got - want) / want;
                if (rel > worst) worst = rel;
                CHECK(rel <= 0x1.0p-40, "u %a: gamma(1/2) %a, z²/2 %a (%g)", u, got, want, rel);
            } else CHECK(std::fabs(got - want) <= 0x1.0p-149, "u %a: gamma(1/2) %a, z²/2 %a", u, got, want);
        }
        std::printf("shape 1/2 against inverseNormalCdf((1 + u)/2)²/2: largest relative difference %.3g\n", worst);
    }
    // P of the root is u again
    for (double shape : shapes) {
        const std::vector<double> c = gammaConsts(shape);
        for (double u : { 0.001, 0.3, 0.5, 0.9, 0.999 }) {
            const double x = fm_inverse_gamma_cdf(shape, c.data(), u);
            if (x < 1e-300) continue;
            CHECK(std::fabs(fm_gamma_p(shape, c[FM_GC_LGAMMA], x) - u) <= 1e-12, "shape %g u %g", shape, u);
        }
    }
    std::printf("OK identities\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "identities") { identities(); return 0; }
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        char* end = nullptr;
        const double first = std::strtod(line, &end);
        if (mode == "exp") std::printf("%a\n", fm_exp64(first));
        else if (mode == "log") std::printf("%a\n", fm_log64(first));
        else if (mode == "icdf" || mode == "p") {
            const double second = std::strtod(end, nullptr);
            if (mode == "p") { std::printf("%a\n", fm_gamma_p(first, gammaConsts(first)[FM_GC_LGAMMA], second)); continue; }
            const std::vector<double> c = gammaConsts(first);
            double again;
            const int steps = halley_steps(first, c.data(), second, &again);
            const double x = fm_inverse_gamma_cdf(first, c.data(), second);
            CHECK(x == again, "the counted loop is not the header's");
            std::printf("%a %d\n", x, steps);
        } else { std::fprintf(stderr, "usage: test_gamma_icdf exp|log|icdf|p|identities\n"); return 2; }
    }
    return 0;
}
