// test_kernel_regression_host.cpp — the host half of the kernel regression (host/kernel_regression.hpp, csrc/kreg_kernel.h) as a program
// of its own, for -fsanitize=address,undefined (tests/test_kernel_regression_cpu.py):
//   * membership: the [a, b) range of fm_kernel_range and of the kernel's two branch-free searches over the padded tables equals the
//     per-pair predicate lower_q < xd && xd < upper_q for keys ON lower_q and upper_q, one ulp to either side, NaN, ±inf, ±0, with duplicated
//     points and bandwidths per point;
//   * a MODEL of fm_kernel_moments_kernel's index arithmetic — grid = binned_blocks(n) x slices, 256 lanes, tiles of 1024 elements read as
//     16-byte groups (the tail into the padding of a vector whose capacity is a multiple of 256 bytes), the slice's range of points, the entry
//     index acc[(q − slice_lo)·qe + term][lane], the wave butterfly, the four waves, the lane-strided partials — over exactly-sized
//     allocations: every out-of-range index is a sanitizer report.  Its sums EQUAL the definition's on dyadic data and lie within
//     2·m·2^-53·Σ|terms| of them on random data;
//   * kernel_local_fit: a straight line is reproduced by order 1, a singular point falls back to order 0, empty points are filled from their
//     neighbours, no fitted point throws.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/kreg_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/kernel_regression.hpp"

using namespace fmhost;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Grid {
    std::vector<double> points, h, lower, upper, rh;
    Grid(std::vector<double> p, std::vector<double> b) : points(std::move(p)), h(std::move(b)), lower(points.size()), upper(points.size()), rh(points.size()) {
        kernel_edges(points.data(), h.data(), (int)points.size(), lower.data(), upper.data(), rh.data());
    }
    int Q() const { return (int)points.size(); }
};

// the kernel's search: binary lifting over a table padded with +inf to FM_KREG_PAD, the first step half the power of two above Q
static uint32_t search_half(uint32_t Q) { uint32_t h = 1; while (2 * h <= Q) h *= 2; return h; }
template <bool STRICT>
static uint32_t count_below(const std::vector<double>& t, uint32_t half0, double xd) {
    uint32_t pos = 0;
    for (uint32_t half = half0; half != 0; half >>= 1) {
        const uint32_t at = pos + half;
        const double v = t.at(at - 1);
        pos = (STRICT ? v < xd : v <= xd) ? at : pos;
    }
    return pos;
}
static std::vector<double> padded(const std::vector<double>& t, size_t to) {
    std::vector<double> p(to, std::numeric_limits<double>::infinity());
    std::copy(t.begin(), t.end(), p.begin());
    return p;
}

static void check_membership(const Grid& g, const std::vector<float>& keys) {
    const int Q = g.Q();
    const uint32_t half0 = search_half((uint32_t)Q);
    REQUIRE(2 * half0 <= (uint32_t)fm::FM_KREG_PAD && 2 * half0 > (uint32_t)Q);
    const std::vector<double> lo = padded(g.lower, 2 * half0 - 1), up = padded(g.upper, 2 * half0 - 1);      // exactly what the search may read
    for (float k : keys) {
        const double xd = (double)k;
        int a, b;
        fm_kernel_range(g.lower.data(), g.upper.data(), Q, xd, &a, &b);
        uint32_t ka = count_below<false>(up, half0, xd), kb = count_below<true>(lo, half0, xd);
        ka = ka < (uint32_t)Q ? ka : (uint32_t)Q; kb = kb < (uint32_t)Q ? kb : (uint32_t)Q;
        for (int q = 0; q < Q; ++q) {
            const bool member = g.lower[(size_t)q] < xd && xd < g.upper[(size_t)q];
            REQUIRE(member == (a <= q && q < b));
            REQUIRE(member == ((int)ka <= q && q < (int)kb));
        }
        if (!(xd - xd == 0.0)) REQUIRE(a >= b && ka >= kb);                      // NaN, ±inf: a member of no point
    }
}

static std::vector<float> edge_keys(const Grid& g) {
    std::vector<float> k = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 0.0f, -0.0f,
                             std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max(), std::numeric_limits<float>::lowest() };
    for (int q = 0; q < g.Q(); ++q)
        for (double e : { g.lower[(size_t)q], g.upper[(size_t)q], g.points[(size_t)q] }) {
            const float f = (float)e;
            k.push_back(f); k.push_back(std::nextafterf(f, INFINITY)); k.push_back(std::nextafterf(f, -INFINITY));
        }
    return k;
}

// ---- the model of the kernel
static double butterfly(std::vector<double> v /* 64 */) {
    for (int off = 32; off > 0; off >>= 1) { std::vector<double> w(64); for (int l = 0; l < 64; ++l) w[(size_t)l] = v[(size_t)l] + v[(size_t)(l ^ off)]; v = w; }
    for (int l = 1; l < 64; ++l) REQUIRE(std::memcmp(&v[0], &v[(size_t)l], 8) == 0 || (v[0] != v[0] && v[(size_t)l] != v[(size_t)l]));      // every lane holds the sum
    return v[0];
}

static std::vector<double> model(const std::vector<float>& key, const std::vector<std::vector<float>>& y, const Grid& g, int kernel, int order) {
    const int64_t n = (int64_t)key.size();
    const uint32_t Q = (uint32_t)g.Q(), ny = (uint32_t)y.size(), qe = (uint32_t)fm_kernel_entries(order, (int)ny);
    fm::DevKernelMomentsArgs A{};
    A.n = n; A.tiles = (uint32_t)((n + fm::FM_KREG_TILE - 1) / fm::FM_KREG_TILE); A.n_points = Q; A.search_half = search_half(Q); A.kernel = (uint32_t)kernel; A.order = (uint32_t)order;
    A.n_y = ny; A.entries_per_point = qe; A.points_per_slice = std::min<uint32_t>(Q, (uint32_t)fm::FM_KREG_ENTRIES / qe); A.n_slices = (Q + A.points_per_slice - 1) / A.points_per_slice;
    uint32_t dummy_counter = 0; uint64_t dummy_flag = 0; double dummy = 0;
    A.counters = &dummy_counter; A.done_flag = &dummy_flag; A.tables = &dummy; A.partials = &dummy; A.out_host = &dummy; A.key = 1; for (uint32_t m = 0; m < ny; ++m) A.y[m] = 1;
    REQUIRE(fm::kernel_moments_shape_ok(A));
    const uint32_t blocks = fm::binned_blocks(n), B = (uint32_t)fm::FM_KREG_BLOCK;
    // vectors as the engine stores them: a capacity that is a multiple of 256 bytes, read in whole 16-byte groups
    const size_t cap = (((size_t)n * 4 + 255) / 256) * 64;
    auto stored = [&](const std::vector<float>& v) { std::vector<float> s(cap, -777.0f); std::copy(v.begin(), v.end(), s.begin()); return s; };
    const std::vector<float> K = stored(key);
    std::vector<std::vector<float>> Y; for (const auto& v : y) Y.push_back(stored(v));
    const std::vector<double> lo = padded(g.lower, (size_t)fm::FM_KREG_PAD), up = padded(g.upper, (size_t)fm::FM_KREG_PAD);
    std::vector<double> out((size_t)Q * qe, -1.0);
    for (uint32_t slice = 0; slice < A.n_slices; ++slice) {
        const uint32_t s_lo = slice * A.points_per_slice, np = Q - s_lo < A.points_per_slice ? Q - s_lo : A.points_per_slice, s_hi = s_lo + np, used = np * qe;
        REQUIRE(used <= (uint32_t)fm::FM_KREG_ENTRIES && s_hi <= Q);
        std::vector<double> part((size_t)fm::FM_KREG_ENTRIES * blocks, -3.0);
        for (uint32_t block = 0; block < blocks; ++block) {
            std::vector<double> acc((size_t)used * B, 0.0);                       // exactly the entries of this slice: a stray entry is a report
            for (uint32_t tile = block; tile < A.tiles; tile += blocks)
                for (uint32_t tid = 0; tid < B; ++tid) {
                    const uint32_t i4 = tile * B + tid;
                    const uint32_t at = (int64_t)i4 * 4 < n ? i4 : 0u;
                    for (int j = 0; j < 4; ++j) {
                        const bool valid = (int64_t)i4 * 4 + j < n;
                        const double xd = (double)K.at((size_t)at * 4 + j);
                        double yd[FM_KERNEL_MAX_Y] = {};
                        for (uint32_t m = 0; m < ny; ++m) yd[m] = (double)Y[m].at((size_t)at * 4 + j);
                        uint32_t a = count_below<false>(up, A.search_half, xd), b = count_below<true>(lo, A.search_half, xd);
                        a = a < Q ? a : Q; b = b < Q ? b : Q;
                        const uint32_t q_lo = a > s_lo ? a : s_lo, q_hi = valid ? (b < s_hi ? b : s_hi) : 0u;
                        for (uint32_t q = q_lo; q < q_hi; ++q) {
                            const double d = xd - g.points.at(q);
                            double terms[FM_KERNEL_MAX_ENTRIES_PER_POINT];
                            fm_kernel_terms(order, (int)ny, fm_kernel_weight(kernel, d, g.rh.at(q)), d, yd, terms);
                            for (uint32_t e = 0; e < qe; ++e) { double& c = acc.at((size_t)((q - s_lo) * qe + e) * B + tid); c = c + terms[e]; }
                        }
                    }
                }
            for (uint32_t e = 0; e < used; ++e) {
                double wave[4];
                for (uint32_t w = 0; w < 4; ++w) wave[w] = butterfly(std::vector<double>(acc.begin() + (size_t)e * B + w * 64, acc.begin() + (size_t)e * B + w * 64 + 64));
                part.at((size_t)e * blocks + block) = ((wave[0] + wave[1]) + wave[2]) + wave[3];
            }
        }
        for (uint32_t e = 0; e < used; ++e) {
            std::vector<double> lanes(64, 0.0);
            for (uint32_t lane = 0; lane < 64; ++lane) for (uint32_t w = lane; w < blocks; w += 64) lanes[lane] += part.at((size_t)e * blocks + w);
            out.at((size_t)s_lo * qe + e) = butterfly(lanes);
        }
    }
    return out;
}

static std::vector<double> definition(const std::vector<float>& key, const std::vector<std::vector<float>>& y, const Grid& g, int kernel, int order) {
    std::vector<const float*> py; for (const auto& v : y) py.push_back(v.data());
    std::vector<double> out((size_t)g.Q() * fm_kernel_entries(order, (int)y.size()));
    kernel_moments_host(key.data(), (int64_t)key.size(), g.points.data(), g.h.data(), g.Q(), kernel, order, py.empty() ? nullptr : py.data(), (int)py.size(), out.data());
    return out;
}

static Grid dyadic_grid(int Q, double h) { std::vector<double> p((size_t)Q); for (int q = 0; q < Q; ++q) p[(size_t)q] = -8.0 + 0.25 * (q / 2 * 2) * (64.0 / Q < 1 ? 0.25 : 1.0); return Grid(p, std::vector<double>((size_t)Q, h)); }

static void check_model() {
    std::mt19937 rng(7);
    for (int64_t n : { 1, 3, 255, 1024, 1025, 4099, 256 * 1024 + 1 }) {
        std::vector<float> key((size_t)n); std::vector<std::vector<float>> y(4, std::vector<float>((size_t)n));
        for (int64_t p = 0; p < n; ++p) {
            key[(size_t)p] = (float)((int)(rng() % 257) - 128) * 0.125f;
            for (auto& v : y) v[(size_t)p] = (float)((int)(rng() % 33) - 16);
        }
        if (n > 8) { key[2] = std::numeric_limits<float>::quiet_NaN(); key[3] = std::numeric_limits<float>::infinity(); key[4] = -std::numeric_limits<float>::infinity(); key[5] = -0.0f; }
        const bool large = n > 100000;
        for (int Q : large ? std::vector<int>{ 37 } : std::vector<int>{ 1, 2, 36, 37, 256 })
            for (int order = 0; order < 2; ++order)
                for (int ny : large ? std::vector<int>{ 1 } : std::vector<int>{ 0, 1, 4 }) {
                    const int kernel = (Q + order + ny) % 5;
                    const Grid g = dyadic_grid(Q, kernel == FM_KERNEL_TRIWEIGHT ? 0.5 : (Q % 2 ? 1.0 : 2.0));
                    const std::vector<std::vector<float>> ys(y.begin(), y.begin() + ny);
                    const std::vector<double> got = model(key, ys, g, kernel, order), want = definition(key, ys, g, kernel, order);
                    if (std::memcmp(got.data(), want.data(), got.size() * 8) != 0) { std::fprintf(stderr, "model differs from the definition: n %lld Q %d order %d ny %d kernel %d\n", (long long)n, Q, order, ny, kernel); std::exit(1); }
                }
    }
    // random data: two summation orders of the same exact terms
    const int64_t n = 20011;
    std::normal_distribution<float> normal(0.0f, 1.0f);
    std::vector<float> key((size_t)n); std::vector<std::vector<float>> y(2, std::vector<float>((size_t)n));
    for (int64_t p = 0; p < n; ++p) { key[(size_t)p] = normal(rng); y[0][(size_t)p] = 2.0f + 3.0f * key[(size_t)p]; y[1][(size_t)p] = normal(rng); }
    std::vector<double> p(41), h(41);
    for (int q = 0; q < 41; ++q) { p[(size_t)q] = -3.0 + 0.15 * q; h[(size_t)q] = 0.3 + 0.004 * std::abs(q - 20); }
    const Grid g(p, h);
    kernelMomentsCheck<const float*>(key.data(), p.data(), h.data(), 41, FM_KERNEL_EPANECHNIKOV, 1, nullptr, 0, &p);
    for (int kernel = 0; kernel < 5; ++kernel) {
        const std::vector<double> got = model(key, y, g, kernel, 1), want = definition(key, y, g, kernel, 1);
        const int qe = fm_kernel_entries(1, 2);
        for (int q = 0; q < 41; ++q) {
            std::vector<double> absolute((size_t)qe, 0.0); int64_t members = 0;
            for (int64_t i = 0; i < n; ++i) {
                const double xd = (double)key[(size_t)i];
                if (!(g.lower[(size_t)q] < xd && xd < g.upper[(size_t)q])) continue;
                ++members;
                const double d = xd - p[(size_t)q], yd[2] = { (double)y[0][(size_t)i], (double)y[1][(size_t)i] };
                double terms[FM_KERNEL_MAX_ENTRIES_PER_POINT];
                fm_kernel_terms(1, 2, fm_kernel_weight(kernel, d, g.rh[(size_t)q]), d, yd, terms);
                for (int e = 0; e < qe; ++e) absolute[(size_t)e] += std::fabs(terms[e]);
            }
            for (int e = 0; e < qe; ++e)
                REQUIRE(std::fabs(got[(size_t)q * qe + e] - want[(size_t)q * qe + e]) <= 2.0 * (double)members * std::ldexp(1.0, -53) * absolute[(size_t)e] * (1.0 + 1e-6));
        }
    }
}

static void check_fit() {
    // a straight line: order 1 reproduces it wherever the 2x2 system is regular
    std::mt19937 rng(11);
    const int64_t n = 5000;
    std::vector<float> key((size_t)n), line((size_t)n);
    std::vector<double> exact((size_t)n);
    for (int64_t p = 0; p < n; ++p) { key[(size_t)p] = (float)((int)(rng() % 1025) - 512) / 256.0f; line[(size_t)p] = 2.0f + 3.0f * key[(size_t)p]; REQUIRE((double)line[(size_t)p] == 2.0 + 3.0 * (double)key[(size_t)p]); }
    std::vector<double> p = { -1.5, -0.5, 0.0, 0.75, 1.5 }, h(5, 0.5);
    const float* py[1] = { line.data() };
    std::vector<double> sums(5 * 5), values(5), slopes(5);
    kernel_moments_host(key.data(), n, p.data(), h.data(), 5, FM_KERNEL_EPANECHNIKOV, 1, py, 1, sums.data());
    kernel_local_fit(sums.data(), 1, 1, p.data(), 5, values.data(), slopes.data());
    for (int q = 0; q < 5; ++q) { REQUIRE(std::fabs(values[(size_t)q] - (2.0 + 3.0 * p[(size_t)q])) <= 1e-12 * 8.0); REQUIRE(std::fabs(slopes[(size_t)q] - 3.0) <= 1e-10); }
    // a singular point (every member at one key: Wdd·W = Wd²) falls back to Wy / W; an empty point is filled from its neighbours
    {
        const double pts[5] = { 0.0, 1.0, 2.0, 3.0, 4.0 };
        double s[5 * 5] = {};
        auto put = [&](int q, double W, double d, double yv) { double* e = s + q * 5; e[0] = W; e[1] = W * d; e[2] = W * d * d; e[3] = W * yv; e[4] = W * d * yv; };
        put(1, 4.0, 0.25, 7.0);                        // singular: det = 0
        put(3, 2.0, -0.5, 11.0);
        double v[5], sl[5];
        kernel_local_fit(s, 1, 1, pts, 5, v, sl);
        REQUIRE(v[1] == 7.0 && sl[1] == 0.0 && v[3] == 11.0);
        REQUIRE(v[0] == 7.0 && v[4] == 11.0 && v[2] == 9.0);      // constant beyond the outermost fitted points, linear between
        double empty[5 * 5] = {};
        bool thrown = false;
        try { kernel_local_fit(empty, 1, 1, pts, 5, v, sl); } catch (const std::invalid_argument&) { thrown = true; }
        REQUIRE(thrown);
        double s0[5 * 2] = { 0, 0, 2.0, 6.0, 0, 0, 0, 0, 4.0, 4.0 };
        kernel_local_fit(s0, 0, 1, pts, 5, v, nullptr);
        REQUIRE(v[0] == 3.0 && v[1] == 3.0 && v[4] == 1.0 && v[2] == 3.0 + (1.0 / 3.0) * (1.0 - 3.0) && v[3] == 3.0 + (2.0 / 3.0) * (1.0 - 3.0));
    }
}

static void check_refusals() {
    const float k[1] = { 0.0f }; double out[16];
    const double fine[2] = { 0.0, 1.0 }, h[2] = { 1.0, 1.0 };
    auto refused = [&](const double* p, const double* b, int Q, int kernel, int order, int ny) {
        const float* y[5] = { k, k, k, k, k };
        try { kernelMomentsCheck<const float*>(k, p, b, Q, kernel, order, y, ny, out); } catch (const std::invalid_argument&) { return true; }
        return false;
    };
    REQUIRE(!refused(fine, h, 2, 0, 0, 0) && !refused(fine, h, 2, 4, 1, 4));
    const double down[2] = { 1.0, 0.0 }, nan_p[2] = { 0.0, std::nan("") }, zero_h[2] = { 1.0, 0.0 }, lower_down[2] = { 1.0, 2.5 }, upper_down[2] = { 2.5, 1.0 };
    REQUIRE(refused(fine, h, 0, 0, 0, 0) && refused(fine, h, 257, 0, 0, 0) && refused(fine, h, 2, 0, 0, 5) && refused(fine, h, 2, 0, 2, 0) && refused(fine, h, 2, 5, 0, 0));
    REQUIRE(refused(down, h, 2, 0, 0, 0) && refused(nan_p, h, 2, 0, 0, 0) && refused(fine, zero_h, 2, 0, 0, 0) && refused(fine, lower_down, 2, 0, 0, 0) && refused(fine, upper_down, 2, 0, 0, 0));
}

int main() {
    static const float some_key[1] = { 0.0f };
    for (int Q : { 1, 2, 3, 36, 37, 63, 64, 255, 256 }) {
        std::vector<double> p((size_t)Q), h((size_t)Q);
        for (int q = 0; q < Q; ++q) { p[(size_t)q] = -1.0 + 0.1 * (q / 2 * 2); h[(size_t)q] = 0.25 + 0.01 * (q % 7 == 0) + 0.001 * q; }      // duplicated points, bandwidths per point
        // per-point bandwidths must keep lower and upper monotone: drop the wiggle where it does not
        bool ok = true;
        try { kernelMomentsCheck<const float*>(some_key, p.data(), h.data(), Q, 0, 0, nullptr, 0, &p); } catch (const std::invalid_argument&) { ok = false; }
        if (!ok) for (int q = 0; q < Q; ++q) h[(size_t)q] = 0.25 + 0.001 * (q / 2 * 2);
        kernelMomentsCheck<const float*>(some_key, p.data(), h.data(), Q, 0, 0, nullptr, 0, &p);
        const Grid g(p, h);
        check_membership(g, edge_keys(g));
        const Grid d = dyadic_grid(Q, 0.5);
        check_membership(d, edge_keys(d));
    }
    check_refusals();
    check_fit();
    check_model();
    std::printf("kernel regression host ok\n");
    return 0;
}
