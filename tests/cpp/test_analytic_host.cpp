// test_analytic_host.cpp — host/normal_functions.hpp under the sanitizers (tests/test_analytic_cpu.py builds it with
// -fsanitize=address,undefined): the argument checks of the two host entry points, and the definitions over the edge list — ±0, ±inf, NaN,
// denormals, the ends of the quantile's domain and beyond, the ends of every piece of the distribution function, arguments whose square
// overflows, degenerate formula elements — with every result checked for the value the contract states.  A stand-alone program.
#include "../../finmath-lib-cuda-extensions_amd/host/normal_functions.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace fmhost;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
template <class F> static bool refuses(F&& f) { try { f(); } catch (const std::invalid_argument&) { return true; } return false; }

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), denorm = std::numeric_limits<float>::denorm_min();
    // ---- the unary functions over the edge list
    const std::vector<float> x = { 0.0f, -0.0f, inf, -inf, nan, denorm, -denorm, 1.17549435e-38f, -1.17549435e-38f, 1.0f, 1.0f - 0x1.0p-24f, -1.0f, 2.0f,
                                   -14.3f, 14.3f, -38.0f, 38.7f, -1e20f, 1e20f, -3.4e38f, 3.4e38f, 0.75f, 1.5f, 2.5f, 3.75f, 5.5f, 8.0f, -8.0f, std::nextafter(-8.0f, 0.0f), std::nextafter(-8.0f, -inf) };
    const int64_t n = (int64_t)x.size();
    const int kinds[4] = { FM_FN_NORMAL_CDF, FM_FN_NORMAL_DENSITY, FM_FN_NORMAL_QUANTILE, FM_FN_NORMAL_CDF };
    std::vector<std::vector<float>> out(4, std::vector<float>((size_t)n, -7.0f));
    float* cols[4] = { out[0].data(), out[1].data(), out[2].data(), out[3].data() };
    function_apply_host(x.data(), n, kinds, 4, cols);
    for (int64_t p = 0; p < n; ++p) {
        const float v = x[(size_t)p], cdf = out[0][(size_t)p], den = out[1][(size_t)p], q = out[2][(size_t)p];
        CHECK(bits(out[3][(size_t)p]) == bits(cdf));                                  // a repeated kind is the same value
        if (v != v) { CHECK(bits(cdf) == 0x7fc00000u && bits(den) == 0x7fc00000u && bits(q) == 0x7fc00000u); continue; }
        CHECK(cdf >= 0.0f && cdf <= 1.0f && den >= 0.0f && den <= 0.3989423f);
        if (v == 0.0f || std::fabs(v) <= 1.17549435e-38f) { CHECK(cdf == 0.5f); CHECK(den == 0.3989423f); }
        if (v == inf) { CHECK(cdf == 1.0f && den == 0.0f); }
        if (v == -inf) { CHECK(cdf == 0.0f && den == 0.0f); }
        if (v <= -14.3f) CHECK(cdf == 0.0f);
        if (v >= 14.3f) CHECK(cdf == 1.0f && den <= denorm);
        if (std::fabs(v) >= 38.7f) CHECK(den == 0.0f);
        if (v < 0.0f || v > 1.0f) CHECK(bits(q) == 0x7fc00000u);
        else if (v == 0.0f) CHECK(q == -inf);
        else if (v == 1.0f) CHECK(q == inf);
        else CHECK(std::isfinite(q) && (q < 0.0f) == (v < 0.5f));
    }
    CHECK(fm_normal_cdf(-38.0) > 0.0 && fm_normal_cdf(-39.0) == 0.0 && fm_normal_cdf(1e300) == 1.0 && fm_normal_cdf(-1e300) == 0.0);
    CHECK(fm_mills_ratio(std::numeric_limits<double>::infinity()) == 0.0);
    for (int i = 0; i < FM_MILLS_PIECES - 1; ++i) {                                   // continuity across a break: the pieces meet within the fit's error
        const double b = FM_MILLS_BREAKS[i], below = fm_mills_ratio(std::nextafter(b, 0.0)), at = fm_mills_ratio(b);
        CHECK(std::fabs(below - at) <= 0x1.0p-45 * at);
    }
    // ---- the refusals of function_apply_host
    CHECK(refuses([&] { function_apply_host(nullptr, n, kinds, 1, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), 0, kinds, 1, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), (int64_t(1) << 31) + 1, kinds, 1, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), n, nullptr, 1, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), n, kinds, 0, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), n, kinds, 5, cols); }));
    CHECK(refuses([&] { function_apply_host(x.data(), n, kinds, 1, nullptr); }));
    { const int bad[1] = { 3 }; CHECK(refuses([&] { function_apply_host(x.data(), n, bad, 1, cols); })); }
    { const int bad[1] = { -1 }; CHECK(refuses([&] { function_apply_host(x.data(), n, bad, 1, cols); })); }
    { float* hole[2] = { out[0].data(), nullptr }; CHECK(refuses([&] { function_apply_host(x.data(), n, kinds, 2, hole); })); }
    // ---- the formulas: degenerate and NaN elements among live ones, every mask, scalars for vectors
    const std::vector<float> F = { 100.0f, 100.0f, 120.0f, 80.0f, 0.0f, -5.0f, 100.0f, nan, 100.0f, 100.0f, inf, 1e-30f };
    const std::vector<float> S = { 0.2f, 0.0f, -0.1f, 0.2f, 0.2f, 0.2f, nan, 0.2f, 0.2f, 1e-6f, 0.2f, 0.2f };
    const std::vector<float> U = { 1.0f, 2.0f, 2.0f, 0.5f, 1.0f, 1.0f, 1.0f, 1.0f, nan, 1.0f, 1.0f, 1.0f };
    const int64_t m = (int64_t)F.size();
    for (int model = 0; model < FM_FORMULA_MODELS; ++model)
        for (int mask = 1; mask <= FM_FORMULA_ALL; ++mask) {
            std::vector<std::vector<float>> o(3, std::vector<float>((size_t)m, -7.0f));
            float* c[3] = { o[0].data(), o[1].data(), o[2].data() };
            option_formula_host(model, F.data(), 0.0, S.data(), 0.0, U.data(), 0.0, m, 1.0, 100.0, mask, c);
            const int at_value = 0, at_delta = mask & 1, at_vega = (mask & 1) + ((mask >> 1) & 1);
            for (int64_t p = 0; p < m; ++p) {
                const bool any_nan = F[(size_t)p] != F[(size_t)p] || S[(size_t)p] != S[(size_t)p] || U[(size_t)p] != U[(size_t)p];
                const bool degenerate = !(S[(size_t)p] > 0.0f) || (model == FM_FORMULA_BLACK_SCHOLES && !(F[(size_t)p] > 0.0f));
                if (mask & FM_FORMULA_VALUE) {
                    const float v = o[at_value][(size_t)p];
                    if (any_nan) CHECK(bits(v) == 0x7fc00000u);
                    else if (degenerate) CHECK(v == U[(size_t)p] * std::fmax(F[(size_t)p] - 100.0f, 0.0f));
                    else CHECK(v >= 0.0f);
                }
                if (mask & FM_FORMULA_DELTA) {
                    const float v = o[at_delta][(size_t)p];
                    if (any_nan) CHECK(bits(v) == 0x7fc00000u);
                    else if (degenerate) CHECK(v == (F[(size_t)p] > 100.0f ? U[(size_t)p] : 0.0f));
                    else CHECK(v >= 0.0f && v <= U[(size_t)p]);
                }
                if (mask & FM_FORMULA_VEGA) {
                    const float v = o[at_vega][(size_t)p];
                    if (any_nan) CHECK(bits(v) == 0x7fc00000u);
                    else if (degenerate) CHECK(v == 0.0f);
                    else if (std::isinf(F[(size_t)p])) CHECK(v >= 0.0f || bits(v) == 0x7fc00000u);      // inf · φ(inf) = inf · 0: what the expression gives, canonical
                    else CHECK(v >= 0.0f);
                }
            }
            for (int f = fm_formula_outputs(mask); f < 3; ++f) CHECK(o[(size_t)f][0] == -7.0f);      // only the asked columns are written
            // T = 0: every element is the limit
            option_formula_host(model, F.data(), 0.0, nullptr, 0.3, nullptr, 2.0, m, 0.0, 100.0, mask, c);
            if (mask & FM_FORMULA_VEGA) for (int64_t p = 0; p < m; ++p) CHECK(F[(size_t)p] != F[(size_t)p] ? bits(o[at_vega][(size_t)p]) == 0x7fc00000u : o[at_vega][(size_t)p] == 0.0f);
        }
    {   // the refusals of option_formula_host
        std::vector<float> o((size_t)m);
        float* c[3] = { o.data(), o.data(), o.data() };
        CHECK(refuses([&] { option_formula_host(2, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 1, c); }));
        CHECK(refuses([&] { option_formula_host(-1, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 1, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, -1.0, 100.0, 1, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, std::nan(""), 100.0, 1, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, (double)inf, 100.0, 1, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, std::nan(""), 1, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 0, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 8, c); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 1, nullptr); }));
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, 0, 1.0, 100.0, 1, c); }));
        float* hole[3] = { o.data(), nullptr, nullptr };
        CHECK(refuses([&] { option_formula_host(0, F.data(), 0, nullptr, 0.2, nullptr, 1, m, 1.0, 100.0, 3, hole); }));
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("analytic host ok\n");
    return 0;
}
