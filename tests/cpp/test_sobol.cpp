// test_sobol.cpp — the C++ host mirror's quasi-Monte-Carlo Brownian motion (host/sobol_brownian_motion.hpp).
//   host    (no device) BrownianMotionFromSobolSequence over the CPU factory: the increments are the definition's, a block behind a path
//           offset is a slice, the bridge's increments of a path add up to its terminal value
//   device  BrownianMotionFromSobolSequenceHip (generated on the device) against BrownianMotionFromSobolSequence over the device factory
//           (drawn on the host, uploaded): every draw EQUAL, both constructions, a block behind an offset
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../finmath-lib-cuda-extensions_amd/host/sobol_brownian_motion.hpp"
#include "../../oracle/host/random_variable_cpu.hpp"

using namespace fmhost;

#define EXPECT(c, what) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, what); std::exit(1); } } while (0)

static const std::vector<double> TIMES = { 0.0, 0.5, 0.6, 2.0, 2.25, 3.0 };

static void host_mode() {
    RandomVariableFloatFactory cpu;
    const TimeDiscretization td(TIMES);
    const int steps = td.getNumberOfTimeSteps();
    for (int construction = 0; construction < 2; ++construction) {
        BrownianMotionFromSobolSequence whole(td, 2, 500, 7, &cpu, construction), part(td, 2, 100, 7, &cpu, construction, true, 400);
        std::vector<double> dt((size_t)steps);
        for (int i = 0; i < steps; ++i) dt[(size_t)i] = td.getTimeStep(i);
        std::vector<double> want((size_t)steps * 2 * 500);
        sobolIncrements(7, 1, construction, steps, 2, 500, 0, dt.data(), want.data());
        for (int i = 0; i < steps; ++i)
            for (int f = 0; f < 2; ++f) {
                const std::vector<double> w = whole.getBrownianIncrement(i, f)->getRealizations(), p = part.getBrownianIncrement(i, f)->getRealizations();
                EXPECT(w.size() == 500 && p.size() == 100, "sizes");
                for (size_t k = 0; k < 500; ++k) EXPECT((float)want[((size_t)i * 2 + f) * 500 + k] == (float)w[k], "the mirror hands out the definition's increments");
                for (size_t k = 0; k < 100; ++k) EXPECT((float)p[k] == (float)w[400 + k], "a block behind an offset is a slice");
                EXPECT(whole.getBrownianIncrement(i, f)->getFiltrationTime() == td.getTime(i + 1), "filtration time");
            }
    }
    std::printf("OK host\n");
}

static void device_mode() {
    check(fmhip_init(0));
    {
        RandomVariableHipFactory factory;
        const TimeDiscretization td(TIMES);
        for (int construction = 0; construction < 2; ++construction)
            for (int randomize = 0; randomize < 2; ++randomize) {
                const int64_t n = 100003;
                BrownianMotionFromSobolSequence host(td, 3, n, 31415, &factory, construction, randomize != 0);
                BrownianMotionFromSobolSequenceHip dev(td, 3, n, 31415, construction, randomize != 0), part(td, 3, 5000, 31415, construction, randomize != 0, 77777);
                for (int i = 0; i < td.getNumberOfTimeSteps(); ++i)
                    for (int f = 0; f < 3; ++f) {
                        const std::vector<double> h = host.getBrownianIncrement(i, f)->getRealizations(), d = dev.getBrownianIncrement(i, f)->getRealizations(), p = part.getBrownianIncrement(i, f)->getRealizations();
                        EXPECT(h.size() == (size_t)n && d.size() == (size_t)n && p.size() == 5000, "sizes");
                        for (size_t k = 0; k < (size_t)n; ++k) EXPECT(std::memcmp(&h[k], &d[k], 8) == 0, "a device draw differs from the host's");
                        for (size_t k = 0; k < 5000; ++k) EXPECT(std::memcmp(&p[k], &d[77777 + k], 8) == 0, "a block behind an offset is a slice");
                    }
            }
    }
    check(fmhip_shutdown());
    std::printf("OK device\n");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "host";
    try {
        if (mode == "host") host_mode();
        else if (mode == "device") device_mode();
        else { std::fprintf(stderr, "usage: test_sobol host|device\n"); return 2; }
    } catch (const std::exception& e) { std::fprintf(stderr, "exception: %s\n", e.what()); return 1; }
    return 0;
}
