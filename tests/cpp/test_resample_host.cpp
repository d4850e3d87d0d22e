// test_resample_host.cpp — the definition of the device resampling (csrc/resample_host.hpp) on the CPU, built with
// -fsanitize=address,undefined by tests/test_resample_cpu.py: the bisection against a linear scan of the definition's predicate for every
// scheme and weight family at sizes around every boundary of the tree; the two consequences the header states (an ancestor has positive
// cleaned weight, 0 <= a_j <= n - 1); a MODEL of the gather kernel as it runs — the table of the chunks' last prefixes, a bisection of it
// and one inside the chunk with the launcher's trip counts — whose every ancestor must be the definition's; and the bisection on hostile
// tables (NaN, descending, infinite prefixes, any target) with exactly-sized heap arrays: it may answer anything, it may not read outside
// [0, last] and it takes exactly `trips` steps.
#include "../../finmath-lib-cuda-extensions_amd/csrc/resample_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace fm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static std::vector<float> weights(int64_t n, int family, std::mt19937& rng)
{
    std::vector<float> w((size_t)n);
    std::uniform_real_distribution<float> uni(0.f, 1.f), expo(-8.f, 8.f);
    for (int64_t p = 0; p < n; ++p) {
        float x;
        switch (family) {
        case 0: x = uni(rng); break;
        case 1: x = std::pow(10.f, expo(rng)); break;                                   // wide range
        case 2: x = (rng() & 1u) ? uni(rng) : 0.f; break;                               // half zeros
        case 3: x = (float)(1u + rng() % 4096u) * 9.313225746154785e-10f; break;        // dyadic
        case 4: x = p == n / 3 ? 1.f : 0.f; break;                                      // one positive weight
        default: {                                                                      // NaN, negative and -0.0 among them
            const uint32_t k = rng() % 8u;
            x = k == 0 ? std::numeric_limits<float>::quiet_NaN() : k == 1 ? -uni(rng) : k == 2 ? -0.f : uni(rng);
        }
        }
        w[(size_t)p] = x;
    }
    if (family == 5) w[(size_t)(n / 2)] = 0.5f;                                         // (at least one positive weight)
    return w;
}

// the definition's ancestor by a linear scan of P
static int64_t scan(const std::vector<double>& P, double t)
{
    const int64_t n = (int64_t)P.size();
    for (int64_t r = 0; r < n; ++r) if (P[(size_t)r] > t) return r;
    for (int64_t r = 0; r < n; ++r) if (P[(size_t)r] == P[(size_t)n - 1]) return r;
    return -1;
}

// the gather kernel's two bisections
static int64_t kernel_model(const std::vector<double>& P, double t)
{
    const int64_t n = (int64_t)P.size(), chunk = prefix_chunk_elems(n);
    const uint32_t blocks = prefix_blocks(n);
    std::vector<double> tops(blocks);
    for (uint32_t c = 0; c < blocks; ++c) tops[c] = P[(size_t)(std::min<int64_t>(((int64_t)c + 1) * chunk, n) - 1)];
    const double total = P[(size_t)n - 1];
    int64_t c = resample_search(tops.data(), 0, (int64_t)blocks, resample_trips((int64_t)blocks), (int64_t)blocks - 1, t, total);
    c = std::min<int64_t>(c, (int64_t)blocks - 1);
    const int64_t lo = c * chunk, len = std::min<int64_t>(chunk, n - lo);
    const int64_t r = resample_search(P.data(), lo, len, resample_trips(std::min(chunk, n)), n - 1, t, total);
    return r < 0 ? 0 : r > n - 1 ? n - 1 : r;
}

int main()
{
    std::mt19937 rng(20261021u);
    CHECK(resample_trips(0) == 0 && resample_trips(1) == 1 && resample_trips(2) == 2 && resample_trips(3) == 2 && resample_trips(4) == 3 && resample_trips(0x7fffffffLL) == 31);
    CHECK(resample_clean(-0.f) == 0.f && !std::signbit(resample_clean(-0.f)) && resample_clean(std::numeric_limits<float>::quiet_NaN()) == 0.f && resample_clean(-1.f) == 0.f && resample_clean(2.f) == 2.f);
    {
        double U = -1.0;
        CHECK(!resample_uniform(std::numeric_limits<float>::quiet_NaN(), U));
        CHECK(resample_uniform(-0.5f, U) && U == 0.0);
        CHECK(resample_uniform(1.0f, U) && U == std::nextafter(1.0, 0.0));
        CHECK(resample_uniform(7.0f, U) && U == std::nextafter(1.0, 0.0));
        CHECK(resample_uniform(std::nextafter(1.0f, 0.0f), U) && U == (double)std::nextafter(1.0f, 0.0f));
        CHECK(resample_degenerate(0.0) && resample_degenerate(-1.0) && resample_degenerate(std::numeric_limits<double>::quiet_NaN()) && resample_degenerate(std::numeric_limits<double>::infinity()) && !resample_degenerate(1e-300));
    }
    const int64_t three = 2 * prefix_chunk_elems(1) + 1;
    const int64_t sizes[] = { 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 3 * 2048 + 5, prefix_chunk_elems(1) + 1, three, three + 4097 };
    for (int64_t n : sizes) {
        for (int family = 0; family < 6; ++family) {
            const std::vector<float> w = weights(n, family, rng);
            std::vector<float> cw((size_t)n);
            for (int64_t r = 0; r < n; ++r) cw[(size_t)r] = resample_clean(w[(size_t)r]);
            std::vector<double> P((size_t)n);
            prefix_sums_host(cw.data(), n, P.data());
            for (int64_t r = 1; r < n; ++r) CHECK(P[(size_t)r] >= P[(size_t)r - 1]);
            const double total = P[(size_t)n - 1];
            if (resample_degenerate(total)) { CHECK(family == 2 || family == 5 || n < 3); continue; }
            std::vector<float> x((size_t)n);
            for (int64_t r = 0; r < n; ++r) x[(size_t)r] = (float)r;
            for (int64_t m : { (int64_t)1, (int64_t)63, (int64_t)65, n, std::max<int64_t>(1, n / 4) }) {
                std::vector<float> u((size_t)m);
                std::uniform_real_distribution<float> uni(0.f, 1.f);
                for (auto& v : u) v = uni(rng);
                if (m > 3) { u[0] = 0.f; u[1] = std::nextafter(1.0f, 0.0f); u[2] = 1.0f; }
                for (int scheme = 0; scheme < 3; ++scheme) {
                    const double offset = scheme == 0 ? (m % 2 ? 0.0 : 0.625) : 0.0;
                    std::vector<float> got((size_t)m);
                    std::vector<int64_t> a((size_t)m, -7);
                    const float* in[1] = { x.data() }; float* out[1] = { got.data() };
                    double tot = -1.0;
                    resample_host(w.data(), n, scheme, m, offset, u.data(), in, 1, out, a.data(), &tot);
                    CHECK(std::memcmp(&tot, &total, 8) == 0);
                    for (int64_t j = 0; j < m; ++j) {
                        double U = 0.0;
                        resample_uniform(u[(size_t)j], U);
                        const double t = resample_target(resample_fraction(scheme, j, m, offset, U), total);
                        const int64_t r = a[(size_t)j];
                        CHECK(t >= 0.0 && t <= total);
                        CHECK(r >= 0 && r <= n - 1);
                        if (r < 0 || r >= n) continue;
                        CHECK(cw[(size_t)r] > 0.f);
                        CHECK(r == scan(P, t));
                        CHECK(r == kernel_model(P, t));
                        CHECK(got[(size_t)j] == (float)r);
                    }
                }
            }
            // targets AT prefixes, one ulp below and above, at the chunk boundaries above all
            const int64_t chunk = prefix_chunk_elems(n);
            for (int64_t r : { (int64_t)0, n - 1, n / 2, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk }) {
                if (r < 0 || r >= n) continue;
                for (double t : { P[(size_t)r], std::nextafter(P[(size_t)r], -1.0), std::nextafter(P[(size_t)r], 1e300) }) {
                    if (!(t >= 0.0 && t <= total)) continue;
                    CHECK(kernel_model(P, t) == scan(P, t));
                    CHECK(resample_search(P.data(), 0, n, resample_trips(n), n - 1, t, total) == scan(P, t));
                }
            }
        }
    }
    // equal weights: the bootstrap
    for (int64_t n : { (int64_t)1, (int64_t)7, (int64_t)4097 }) {
        std::vector<float> x((size_t)n), u = { 0.f, 0.5f, std::nextafter(1.0f, 0.0f), 1.0f, -3.f, std::numeric_limits<float>::quiet_NaN() }, got(u.size());
        for (int64_t r = 0; r < n; ++r) x[(size_t)r] = (float)(r + 1);
        std::vector<int64_t> a(u.size());
        const float* in[1] = { x.data() }; float* out[1] = { got.data() };
        double tot = 0;
        resample_host(nullptr, n, FM_RESAMPLE_MULTINOMIAL, (int64_t)u.size(), 0.0, u.data(), in, 1, out, a.data(), &tot);
        CHECK(tot == (double)n);
        for (size_t j = 0; j + 1 < u.size(); ++j) {
            const double U = u[j] < 0 ? 0.0 : u[j] >= 1.f ? std::nextafter(1.0, 0.0) : (double)u[j];
            CHECK(a[j] == std::min<int64_t>((int64_t)std::floor(U * (double)n), n - 1) && got[j] == x[(size_t)a[j]]);
        }
        uint32_t bits; std::memcpy(&bits, &got.back(), 4);
        CHECK(a.back() == -1 && bits == FM_RESAMPLE_NAN_BITS);
    }
    // hostile tables: any content, any target — the search stays inside [0, last] (exactly-sized heap arrays: ASan is the check)
    for (int round = 0; round < 2000; ++round) {
        const int64_t n = 1 + (int64_t)(rng() % 300u);
        std::vector<double> P((size_t)n);
        for (auto& p : P) { const uint32_t k = rng() % 6u; p = k == 0 ? std::numeric_limits<double>::quiet_NaN() : k == 1 ? std::numeric_limits<double>::infinity() : k == 2 ? -1.0 : (double)(rng() % 100u); }
        const double ts[] = { 0.0, -1.0, 1e300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), (double)(rng() % 100u) };
        for (double t : ts) {
            const int64_t lo = (int64_t)(rng() % (uint32_t)n), len = 1 + (int64_t)(rng() % (uint32_t)(n - lo));
            const int64_t r = resample_search(P.data(), lo, len, resample_trips(len) + (int)(rng() % 3u), n - 1, t, P[(size_t)n - 1]);
            CHECK(r >= lo && r <= lo + len);
        }
    }
    // refusals of the definition
    {
        float one = 1.f, got = 0.f; const float* in[1] = { &one }; float* out[1] = { &got }; int64_t a = 0;
        auto refused = [&](auto&& call) { try { call(); } catch (const std::invalid_argument&) { return true; } return false; };
        CHECK(refused([&] { resample_host(&one, 1, 3, 1, 0.0, &one, in, 1, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 0, 0, 0.0, nullptr, in, 1, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 0, 0, 1, 0.0, nullptr, in, 1, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 0, 1, 1.0, nullptr, in, 1, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 0, 1, 0.0, nullptr, in, 9, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 0, 1, 0.0, nullptr, nullptr, 0, nullptr, nullptr, nullptr); }));
        CHECK(refused([&] { resample_host(nullptr, 1, 0, 1, 0.0, nullptr, nullptr, 0, nullptr, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 2, 1, 0.0, nullptr, in, 1, out, &a, nullptr); }));
        CHECK(refused([&] { resample_host(&one, 1, 0, 1, 0.0, nullptr, nullptr, 1, out, &a, nullptr); }));
        CHECK(got == 0.f && a == 0);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("resample host ok\n");
    return 0;
}
