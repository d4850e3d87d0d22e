// test_prefix_host.cpp — the host half of the device prefix sums (csrc/prefix_host.hpp) on the CPU, built with -fsanitize=address,undefined
// by tests/test_prefix_cpu.py: the chunk arithmetic for n around every boundary up to 2^31 - 1 (the chunks cover the tiles once, no
// workgroup is empty, at most FM_PREFIX_MAX_BLOCKS rows, a chunk is at least two tiles, positions stay below 2^32), the definition against
// a long-double sum within the published bound and for monotonicity on wide-range weights, and a MODEL of the three kernels as they run —
// elements past n enter as -0.0, a lane scans its 8 elements, the bases of a level are a serial chain over the subunits' last prefixes,
// totals { total, largest } per chunk, the carry over the rows with the chunk of every query, apply / query — whose every P[r], every
// out[r] and every answer must be the definition's, bit for bit.
#include "../../finmath-lib-cuda-extensions_amd/csrc/prefix_host.hpp"

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

static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }      // of a NaN only that it is one
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }

static std::vector<float> sample(int64_t n, int family, std::mt19937& rng)
{
    std::vector<float> a((size_t)n);
    std::normal_distribution<float> normal(0.f, 1.f);
    std::uniform_real_distribution<float> uni(0.f, 1.f), expo(-8.f, 8.f);
    for (int64_t p = 0; p < n; ++p) {
        float x;
        switch (family) {
        case 0: x = uni(rng); break;
        case 1: x = normal(rng); break;
        case 2: x = std::pow(10.f, expo(rng)); break;                                   // wide range, non-negative: 1e-8 … 1e8
        case 3: x = std::pow(10.f, expo(rng)) * ((rng() & 1u) ? 1.f : -1.f); break;     // wide range, signed
        case 4: x = (float)(rng() % 4096u) * 9.313225746154785e-10f; break;             // dyadic: integers below 2^12 times 2^-30
        case 5: x = std::max(normal(rng) - 0.2f, 0.f); break;                           // half zeros
        default: {
            const uint32_t r = rng() % 64u;
            x = r == 0 ? std::numeric_limits<float>::infinity() : r == 1 ? -std::numeric_limits<float>::infinity()
              : r == 2 ? std::numeric_limits<float>::quiet_NaN() : r == 3 ? -0.f : normal(rng);
        }
        }
        a[(size_t)p] = x;
    }
    return a;
}

static void check_chunks(int64_t n)
{
    const int64_t tiles = prefix_tiles(n);
    const uint32_t chunk = prefix_chunk_tiles(n), blocks = prefix_blocks(n);
    CHECK(tiles >= 1 && tiles * FM_PREFIX_TILE >= n && (tiles - 1) * FM_PREFIX_TILE < n);
    CHECK(chunk >= (uint32_t)FM_PREFIX_MIN_CHUNK_TILES && blocks >= 1u && blocks <= (uint32_t)FM_PREFIX_MAX_BLOCKS);
    CHECK((int64_t)blocks * chunk >= tiles && ((int64_t)blocks - 1) * chunk < tiles);      // every tile once, no workgroup empty
    CHECK((uint64_t)n + FM_PREFIX_TILE < (1ull << 32));
    CHECK((uint64_t)chunk * FM_PREFIX_TILE <= (1ull << 31));                               // the carry kernel's uint32 chunk size
    CHECK(prefix_chunk_elems(n) == (int64_t)chunk * FM_PREFIX_TILE);
    CHECK(prefix_chain(n) == 24 + (int)chunk - 1 + (int)blocks - 1);
    CHECK(prefix_scratch_bytes(n, 4096) % 256 == 0 && prefix_rows_bytes(n) >= blocks * sizeof(PrefixRow) && prefix_bases_bytes(n) >= (blocks + 1) * 8);
}

// ---------------------------------------------------------------- the kernels' model
struct Model {
    const std::vector<float>& v; int64_t n; uint32_t chunk_tiles, blocks;
    std::vector<PrefixRow> rows; std::vector<double> bases; double whole = 0;
    explicit Model(const std::vector<float>& a) : v(a), n((int64_t)a.size()), chunk_tiles(prefix_chunk_tiles(n)), blocks(prefix_blocks(n)), rows(blocks), bases(blocks + 1) {}

    // pf_tile: the tile's prefixes inside the chunk, p[FM_PREFIX_TILE]
    void tile(int64_t t, bool first_tile, double& carry, double* p) const
    {
        double last[FM_PREFIX_BLOCK];
        for (int tid = 0; tid < FM_PREFIX_BLOCK; ++tid) {
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
                const int64_t e = t * FM_PREFIX_TILE + (int64_t)tid * FM_PREFIX_ITEMS + i;
                const double x = e < n ? (double)v[(size_t)e] : -0.0;
                p[tid * FM_PREFIX_ITEMS + i] = i == 0 ? x : p[tid * FM_PREFIX_ITEMS + i - 1] + x;
            }
            last[tid] = p[tid * FM_PREFIX_ITEMS + FM_PREFIX_ITEMS - 1];
        }
        auto add_base = [&](int tid, double base) { for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[tid * FM_PREFIX_ITEMS + i] = base + p[tid * FM_PREFIX_ITEMS + i]; };
        double group_last[FM_PREFIX_BLOCK / FM_PREFIX_GROUP], wave_last[FM_PREFIX_WAVES];
        for (int g = 0; g < FM_PREFIX_BLOCK / FM_PREFIX_GROUP; ++g) {
            double run = last[g * FM_PREFIX_GROUP];
            for (int k = 1; k < FM_PREFIX_GROUP; ++k) { add_base(g * FM_PREFIX_GROUP + k, run); run = run + last[g * FM_PREFIX_GROUP + k]; }
            group_last[g] = run;
        }
        for (int w = 0; w < FM_PREFIX_WAVES; ++w) {
            double run = group_last[w * FM_PREFIX_GROUPS];
            for (int g = 1; g < FM_PREFIX_GROUPS; ++g) {
                for (int k = 0; k < FM_PREFIX_GROUP; ++k) add_base((w * FM_PREFIX_GROUPS + g) * FM_PREFIX_GROUP + k, run);
                run = run + group_last[w * FM_PREFIX_GROUPS + g];
            }
            wave_last[w] = run;
        }
        double run = wave_last[0];
        for (int w = 1; w < FM_PREFIX_WAVES; ++w) { for (int l = 0; l < 64; ++l) add_base(w * 64 + l, run); run = run + wave_last[w]; }
        if (first_tile) carry = run;
        else { for (int i = 0; i < FM_PREFIX_TILE; ++i) p[i] = carry + p[i]; carry = carry + run; }
    }
    static double larger(double a, double b) { return (b > a || a != a) ? b : a; }
    void totals()
    {
        std::vector<double> p(FM_PREFIX_TILE);
        const int64_t tiles = prefix_tiles(n);
        for (uint32_t w = 0; w < blocks; ++w) {
            const int64_t t0 = (int64_t)w * chunk_tiles, t1 = std::min<int64_t>(t0 + chunk_tiles, tiles);
            double carry = 0.0, largest = std::numeric_limits<double>::quiet_NaN();
            for (int64_t t = t0; t < t1; ++t) { tile(t, t == t0, carry, p.data()); for (double x : p) largest = larger(largest, x); }
            rows[w] = PrefixRow{ carry, largest };
        }
    }
    void carry()
    {
        double run = rows[0].total;
        for (uint32_t c = 1; c < blocks; ++c) { bases[c] = run; run = run + rows[c].total; }
        whole = bases[blocks] = run;
    }
    uint32_t locate(double t) const
    {
        uint32_t c = 0;
        for (; c < blocks; ++c) { const double top = c == 0 ? rows[0].largest : bases[c] + rows[c].largest; if (top >= t) break; }
        return c;
    }
    // the apply kernel: every P[r]
    std::vector<double> apply() const
    {
        std::vector<double> P((size_t)n), p(FM_PREFIX_TILE);
        const int64_t tiles = prefix_tiles(n);
        for (uint32_t w = 0; w < blocks; ++w) {
            const int64_t t0 = (int64_t)w * chunk_tiles, t1 = std::min<int64_t>(t0 + chunk_tiles, tiles);
            double carry = 0.0;
            for (int64_t t = t0; t < t1; ++t) {
                tile(t, t == t0, carry, p.data());
                for (int i = 0; i < FM_PREFIX_TILE && t * FM_PREFIX_TILE + i < n; ++i) P[(size_t)(t * FM_PREFIX_TILE + i)] = w == 0 ? p[i] : bases[w] + p[i];
            }
        }
        return P;
    }
    // the query kernel for one threshold: (position, sum)
    std::pair<int64_t, double> search(double t) const
    {
        const uint32_t c = locate(t);
        if (c >= blocks) return { n, whole };
        std::vector<double> p(FM_PREFIX_TILE);
        const int64_t tiles = prefix_tiles(n), t0 = (int64_t)c * chunk_tiles, t1 = std::min<int64_t>(t0 + chunk_tiles, tiles);
        double carry = 0.0;
        for (int64_t tl = t0; tl < t1; ++tl) {
            tile(tl, tl == t0, carry, p.data());
            for (int i = 0; i < FM_PREFIX_TILE && tl * FM_PREFIX_TILE + i < n; ++i) { const double P = c == 0 ? p[i] : bases[c] + p[i]; if (P >= t) return { tl * FM_PREFIX_TILE + i, P }; }
        }
        CHECK(!"a located chunk holds its crossing");
        return { n, whole };
    }
};

static void check_model(const std::vector<float>& a, std::mt19937& rng)
{
    const int64_t n = (int64_t)a.size();
    std::vector<double> def((size_t)n);
    prefix_sums_host(a.data(), n, def.data());
    Model m(a);
    m.totals(); m.carry();
    const std::vector<double> P = m.apply();
    bool equal = true;
    for (int64_t r = 0; r < n; ++r) equal &= same(P[(size_t)r], def[(size_t)r]);
    CHECK(equal);
    CHECK(same(m.whole, def[(size_t)n - 1]));
    for (int mode = 0; mode < 2; ++mode) { bool eq = true; for (int64_t r = 0; r < n; r += 7) eq &= same(prefix_out_host(P[(size_t)r], r, mode), mode ? (float)(def[(size_t)r] / (double)(r + 1)) : (float)def[(size_t)r]); CHECK(eq); }
    // thresholds at, just below and just above prefixes; below everything; above everything; NaN
    std::vector<double> ts = { -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), 0.0, def[0] };
    for (int k = 0; k < 24; ++k) { const double x = def[(size_t)(rng() % (uint64_t)n)]; ts.push_back(x); ts.push_back(std::nextafter(x, -1e300)); ts.push_back(std::nextafter(x, 1e300)); }
    for (double t : ts) {
        const auto got = m.search(t);
        const int64_t want = prefix_search_host(def.data(), n, t);
        CHECK(got.first == want);
        CHECK(same(got.second, want < n ? def[(size_t)want] : def[(size_t)n - 1]));
    }
}

int main()
{
    // chunk arithmetic around every boundary
    const int64_t tile = FM_PREFIX_TILE, full = (int64_t)FM_PREFIX_MAX_BLOCKS * FM_PREFIX_MIN_CHUNK_TILES * tile;
    std::vector<int64_t> ns = { 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 4 * tile, 4 * tile + 1,
                                100003, full - 1, full, full + 1, full + tile, full + tile + 1, 3 * full / 2, 3 * full / 2 + 1, 2 * full, 2 * full + 1,
                                (int64_t)1 << 26, ((int64_t)1 << 30) + 1, FM_PREFIX_MAX_N - tile, FM_PREFIX_MAX_N - 1, FM_PREFIX_MAX_N };
    for (int64_t k = 1; k <= 1024; k += 93) { ns.push_back(k * full - 1); ns.push_back(k * full); ns.push_back(k * full + 1); }
    for (int64_t n : ns) if (prefix_size_ok(n)) check_chunks(n);
    CHECK(!prefix_size_ok(0) && !prefix_size_ok(-1) && !prefix_size_ok(FM_PREFIX_MAX_N + 1) && prefix_size_ok(FM_PREFIX_MAX_N));
    CHECK(prefix_blocks(FM_PREFIX_MAX_N) == 1024u && prefix_chunk_tiles(FM_PREFIX_MAX_N) == 1024u);
    CHECK(prefix_blocks(2 * tile) == 1u && prefix_blocks(2 * tile + 1) == 2u && prefix_blocks(4 * tile + 1) == 3u);
    CHECK(prefix_chunk_tiles(full) == 2u && prefix_chunk_tiles(full + 1) == 3u);
    {   // the definition's refusals
        float x = 1.f; double p = 0;
        int thrown = 0;
        try { prefix_sums_host(nullptr, 1, &p); } catch (const std::invalid_argument&) { ++thrown; }
        try { prefix_sums_host(&x, 1, nullptr); } catch (const std::invalid_argument&) { ++thrown; }
        try { prefix_sums_host(&x, 0, &p); } catch (const std::invalid_argument&) { ++thrown; }
        try { prefix_sums_host(&x, FM_PREFIX_MAX_N + 1, &p); } catch (const std::invalid_argument&) { ++thrown; }
        CHECK(thrown == 4);
    }

    std::mt19937 rng(20240611u);
    const int64_t sizes[] = { 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1, 4 * tile + 77, 100003 };
    for (int64_t n : sizes)
        for (int family = 0; family < 7; ++family) {
            const std::vector<float> a = sample(n, family, rng);
            check_model(a, rng);
            std::vector<double> def((size_t)n);
            prefix_sums_host(a.data(), n, def.data());
            if (family == 6) continue;
            // accuracy within the published bound, against a long-double running sum; monotone for input without negative elements
            long double exact = 0.0L, mass = 0.0L;
            bool within = true, monotone = true;
            for (int64_t r = 0; r < n; ++r) {
                exact += (long double)a[(size_t)r]; mass += std::fabs((long double)a[(size_t)r]);
                // (the long-double sum itself: at most n·2^-64·mass away from the exact one)
                within &= std::fabs((long double)def[(size_t)r] - exact) <= ((long double)(prefix_chain(n) + 1) * 0x1p-53L + (long double)n * 0x1p-63L) * mass;
                if (r > 0) monotone &= def[(size_t)r] >= def[(size_t)r - 1];
            }
            CHECK(within);
            if (family == 0 || family == 2 || family == 4 || family == 5) CHECK(monotone);
            if (family == 4) {      // dyadic: every order gives the same bits
                double run = 0.0; bool eq = true;
                for (int64_t r = 0; r < n; ++r) { run += (double)a[(size_t)r]; eq &= run == def[(size_t)r]; }
                CHECK(eq);
            }
        }
    {   // a model over a chunk of three tiles (one n just past a full row table), and the edge inputs
        const int64_t n = full + 5;
        std::vector<float> a = sample(n, 3, rng);
        check_model(a, rng);
        std::vector<float> z(5000, 0.f); z[0] = -0.f; z[1] = -0.f;
        std::vector<double> def(z.size());
        prefix_sums_host(z.data(), (int64_t)z.size(), def.data());
        CHECK(std::signbit(def[0]) && std::signbit(def[1]) && !std::signbit(def[2]) && !std::signbit(def.back()));
        check_model(z, rng);
        for (int64_t at : { (int64_t)0, (int64_t)7, (int64_t)8, (int64_t)63, (int64_t)64, (int64_t)511, (int64_t)512, tile - 1, tile, 2 * tile - 1, 2 * tile, 4 * tile }) {
            std::vector<float> b = sample(4 * tile + 9, 0, rng);
            b[(size_t)at] = std::numeric_limits<float>::quiet_NaN();
            std::vector<double> d(b.size());
            prefix_sums_host(b.data(), (int64_t)b.size(), d.data());
            bool ok = true;
            for (int64_t r = 0; r < (int64_t)b.size(); ++r) ok &= (d[(size_t)r] != d[(size_t)r]) == (r >= at);
            CHECK(ok);
            check_model(b, rng);
            b[(size_t)at] = std::numeric_limits<float>::infinity();
            if (at + 1 < (int64_t)b.size()) b[(size_t)at + 1] = -std::numeric_limits<float>::infinity();
            prefix_sums_host(b.data(), (int64_t)b.size(), d.data());
            CHECK(d[(size_t)at] == std::numeric_limits<double>::infinity() && d[(size_t)at + 1] != d[(size_t)at + 1] && d.back() != d.back());
            check_model(b, rng);
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("prefix host ok\n");
    return 0;
}
