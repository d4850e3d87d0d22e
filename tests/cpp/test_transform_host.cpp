// test_transform_host.cpp — host/transform_formula.hpp under the sanitizers (tests/test_transform_formula_cpu.py builds it with
// -fsanitize=address,undefined): every refusal of the argument check, and the definition over every line of its semantics — a NaN in each
// operand, forwards and strikes that are zero, negative, −0, denormal or infinite, a state that overflows the exponent, an argument of the
// sine beyond its range — and over a sweep of bit patterns as operands with tables of 1, 2 and 256 nodes.  A stand-alone program.
#include "../../finmath-lib-cuda-extensions_amd/host/transform_formula.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace fmhost;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static uint64_t bits64(double f) { uint64_t b; std::memcpy(&b, &f, 8); return b; }
static const uint64_t NAN64 = 0x7ff8000000000000ull;
template <class F> static bool refuses(F&& f) { try { f(); } catch (const std::invalid_argument&) { return true; } return false; }
static bool all_nan(const FmTransformOut& r) { return bits64(r.value) == NAN64 && bits64(r.delta) == NAN64 && bits64(r.state_delta) == NAN64; }

// a Black–Scholes-like table with a state: a_re = −w(u² + ¼)/2 + ln(weight), b = −(u² + ¼)/2 − 0.1·u·i per unit of the state
static std::vector<double> table(int J, int S, double w)
{
    std::vector<double> t((size_t)J * (size_t)(3 + 2 * S));
    for (int j = 0; j < J; ++j) {
        double* row = t.data() + (size_t)j * (size_t)(3 + 2 * S);
        const double u = 40.0 * (j + 0.5) / J, h = 40.0 / J;
        row[0] = u; row[1] = -0.5 * w * (u * u + 0.25) + std::log(h / (3.14159265358979323846 * (u * u + 0.25))); row[2] = 0.0;
        for (int s = 0; s < S; ++s) { row[3 + s] = -0.5 * (u * u + 0.25) / (s + 1); row[3 + S + s] = -0.1 * u; }
    }
    return t;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan(""), denormal = (double)std::numeric_limits<float>::denorm_min();
    // ---- the argument check
    {
        std::vector<double> t = table(8, 1, 0.04);
        float f[4] = { 90.0f, 100.0f, 110.0f, 120.0f }, o0[4], o1[4], o2[4];
        float* out[3] = { o0, o1, o2 };
        const float* states[1] = { nullptr };
        const float* state_vectors[1] = { f };
        double scalars[1] = { 0.04 };
        auto call = [&](const double* nodes, int J, int S, const float* forward, const float* const* st, const double* sc, const float* unit, int64_t n, double K, int mask, float* const* o) {
            transform_option_host(nodes, J, S, forward, 100.0, st, sc, unit, 1.0, n, K, mask, o);
        };
        CHECK(!refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(!refuses([&] { call(t.data(), 8, 1, nullptr, state_vectors, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 0, 1, f, states, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 257, 1, f, states, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 8, -1, f, states, scalars, nullptr, 4, 100.0, 3, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 3, f, states, scalars, nullptr, 4, 100.0, 3, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 0, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 8, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 0, f, nullptr, nullptr, nullptr, 4, 100.0, 4, out); }));          // the state delta without a state
        CHECK(!refuses([&] { call(table(8, 0, 0.04).data(), 8, 0, f, nullptr, nullptr, nullptr, 4, 100.0, 3, out); }));
        CHECK(refuses([&] { call(nullptr, 8, 1, f, states, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, nullptr, scalars, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, nullptr, nullptr, 4, 100.0, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 7, nullptr); }));
        float* holed[3] = { o0, nullptr, o2 };
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 7, holed); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, nullptr, states, scalars, nullptr, 4, 100.0, 7, out); }));      // no vector operand
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, nan, 7, out); }));
        CHECK(refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 0, 100.0, 7, out); }));
        for (double bad : { nan, inf, -inf }) {
            std::vector<double> b = t;
            b[17] = bad;
            CHECK(refuses([&] { call(b.data(), 8, 1, f, states, scalars, nullptr, 4, 100.0, 7, out); }));
        }
        CHECK(!refuses([&] { call(t.data(), 8, 1, f, states, scalars, nullptr, 4, inf, 7, out); }));             // an infinite strike is no NaN: the sum's own arithmetic
    }
    // ---- the semantics, in doubles
    for (int S = 0; S <= 2; ++S) {
        const std::vector<double> t = table(64, S, 0.04);
        const double V0 = 0.02, V1 = 0.01, K = 100.0, N = 0.5;
        CHECK(all_nan(fm_transform_option(t.data(), 64, S, nan, N, V0, V1, K)) && all_nan(fm_transform_option(t.data(), 64, S, 100.0, nan, V0, V1, K)));
        CHECK(all_nan(fm_transform_option(t.data(), 64, S, 100.0, N, V0, V1, nan)));
        CHECK(all_nan(fm_transform_option(t.data(), 64, S, 100.0, N, nan, V1, K)) == (S >= 1) && all_nan(fm_transform_option(t.data(), 64, S, 100.0, N, V0, nan, K)) == (S >= 2));
        for (double F : { 0.0, -0.0, -5.0, -inf }) {
            const FmTransformOut r = fm_transform_option(t.data(), 64, S, F, N, V0, V1, K);
            CHECK(r.value == 0.0 && r.delta == 0.0 && r.state_delta == 0.0);
        }
        for (double strike : { 0.0, -0.0, -5.0 }) {
            const FmTransformOut r = fm_transform_option(t.data(), 64, S, 120.0, N, V0, V1, strike);
            CHECK(r.value == N * (120.0 - strike) && r.delta == N && r.state_delta == 0.0);
        }
        { const FmTransformOut r = fm_transform_option(t.data(), 64, S, 100.0, N, V0, V1, -inf); CHECK(r.value == inf && r.delta == N && r.state_delta == 0.0); }
        // live: inside the arbitrage bounds, a delta in (0, 1)·N, and for a table whose b_re is negative a state delta above 0
        for (double F : { 60.0, 100.0, 160.0 }) {
            const FmTransformOut r = fm_transform_option(t.data(), 64, S, F, N, V0, V1, K);
            CHECK(r.value > N * (F > K ? F - K : 0.0) && r.value < N * F && r.delta > 0.0 && r.delta < N);
            if (S >= 1) CHECK(r.state_delta > 0.0); else CHECK(r.state_delta == 0.0);
        }
        // the smallest fp32 denormal as a forward is live: ln(F/K) is finite and so is every output (the sum is not clamped: no bound is claimed)
        { const FmTransformOut r = fm_transform_option(t.data(), 64, S, denormal, N, V0, V1, K); CHECK(r.value - r.value == 0.0 && r.delta - r.delta == 0.0 && r.state_delta - r.state_delta == 0.0); }
        // an infinite forward: k = +∞, u·k beyond the sine's range: NaN
        CHECK(fm_transform_option(t.data(), 64, S, inf, N, V0, V1, K).value != fm_transform_option(t.data(), 64, S, inf, N, V0, V1, K).value);
        if (S >= 1) {
            // a state that overflows e: E = +∞, and ∞·cos or ∞ − ∞ is a NaN or an infinity; nothing is clamped, nothing traps
            const FmTransformOut r = fm_transform_option(t.data(), 64, S, 100.0, N, -1e300, V1, K);
            CHECK(!(r.value - r.value == 0.0));
            CHECK(bits(fm_narrow(fm_double(NAN64))) == 0x7fc00000u);
            // … and one that takes θ beyond FM_TRIG_MAX (b_im = −0.1·u, u up to 40): a NaN
            std::vector<double> tame = t;
            for (int j = 0; j < 64; ++j) tame[(size_t)j * (3 + 2 * S) + 3] = 0.0;
            CHECK(all_nan(fm_transform_option(tame.data(), 64, S, 100.0, N, 1e7, V1, K)));
        }
    }
    // ---- a sweep of bit patterns as operands: no trap, no sanitizer report, and a NaN comes back as THE quiet NaN
    {
        uint64_t state = 0x243f6a8885a308d3ull;
        for (int J : { 1, 2, 256 }) {
            const std::vector<double> t = table(J, 2, 0.09);
            std::vector<float> F(512), N(512), A(512), B(512), o0(512), o1(512), o2(512);
            for (int i = 0; i < 512; ++i) {
                float* dst[4] = { &F[i], &N[i], &A[i], &B[i] };
                for (float* d : dst) { state = state * 6364136223846793005ull + 1442695040888963407ull; const uint32_t b = (uint32_t)(state >> 32); std::memcpy(d, &b, 4); }
            }
            const float* states[2] = { A.data(), B.data() };
            const double scalars[2] = { 0.0, 0.0 };
            float* out[3] = { o0.data(), o1.data(), o2.data() };
            transform_option_host(t.data(), J, 2, F.data(), 0.0, states, scalars, N.data(), 0.0, 512, 100.0, 7, out);
            for (int i = 0; i < 512; ++i) for (float* o : out) if (o[i] != o[i]) CHECK(bits(o[i]) == 0x7fc00000u);
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("transform host ok\n");
    return 0;
}
