// test_trig64_host.cpp — host/trig64.hpp under the sanitizers (tests/test_transform_formula_cpu.py builds it with
// -fsanitize=address,undefined): the range's ends, the special arguments, the symmetry bit for bit over a sweep of bit patterns, and the
// contract's bound against the C library's sine and cosine (correct to an ulp: loose by that ulp only).  A stand-alone program.
#include "../../finmath-lib-cuda-extensions_amd/host/trig64.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

using namespace fmhost;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint64_t bits64(double f) { uint64_t b; std::memcpy(&b, &f, 8); return b; }
static double from_bits(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
static const uint64_t NAN64 = 0x7ff8000000000000ull, SIGN = 0x8000000000000000ull;

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    for (double x : { inf, -inf, nan, std::nextafter(FM_TRIG_MAX, inf), -std::nextafter(FM_TRIG_MAX, inf), 1e300, -1e300 }) {
        const FmSinCos r = fm_sincos64(x);
        CHECK(bits64(r.sin) == NAN64 && bits64(r.cos) == NAN64);
    }
    { const FmSinCos r = fm_sincos64(0.0); CHECK(bits64(r.sin) == 0 && r.cos == 1.0); }
    { const FmSinCos r = fm_sincos64(-0.0); CHECK(bits64(r.sin) == SIGN && r.cos == 1.0); }
    { const FmSinCos r = fm_sincos64(FM_TRIG_MAX); CHECK(r.sin == r.sin && r.cos == r.cos); }
    const double bound = (FM_TRIG_ERROR_ULPS + 1.0) * 0x1p-53;
    uint64_t state = 0x9e3779b97f4a7c15ull;
    double worst = 0.0;
    for (int i = 0; i < 2000000; ++i) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        // every exponent up to the range's end, random mantissas
        const uint64_t exponent = (state >> 52) % (1023 + 20);
        double x = from_bits((exponent << 52) | (state & 0x000fffffffffffffull));
        if (x > FM_TRIG_MAX) x = FM_TRIG_MAX;
        const FmSinCos p = fm_sincos64(x), m = fm_sincos64(-x);
        CHECK(bits64(m.sin) == (bits64(p.sin) ^ SIGN) && bits64(m.cos) == bits64(p.cos));
        const double es = std::fabs(p.sin - std::sin(x)), ec = std::fabs(p.cos - std::cos(x));
        if (es > worst) worst = es;
        if (ec > worst) worst = ec;
        CHECK(es <= bound && ec <= bound);
        if (failures > 20) break;
    }
    std::printf("worst absolute error against the C library: %.3f * 2^-53\n", worst * 0x1p53);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("trig64 host ok\n");
    return 0;
}
