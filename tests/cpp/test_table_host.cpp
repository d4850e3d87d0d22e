// test_table_host.cpp — the host half of table_kernel.hip, stand-alone under AddressSanitizer / UBSan (tests/test_table_cpu.py builds and runs
// it): the coarse index of host/tabulated_function.hpp against the plain search, with X on and one ulp beside every cell boundary and every
// knot; an index that is wrong on purpose (the correction against K[s−1] and K[s] still finds the definition's s); and a model of the
// kernel's loop — whole 16-byte groups, the capped grid's wrap, the tail into the padding of a buffer whose capacity is a multiple of 256
// bytes — over exactly-sized allocations, compared with the definition (table_apply_host).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/table_kernel.h"

using namespace fmhost;

static void die(const char* what, long a, long b) { std::fprintf(stderr, "%s: %ld, %ld\n", what, a, b); std::exit(1); }

static std::vector<double> knots_of(int m, int kind) {
    std::vector<double> k((size_t)m);
    for (int i = 0; i < m; ++i)
        k[(size_t)i] = kind == 0 ? -3.0 + 0.1 * i : kind == 1 ? 1e-6 * std::pow(1e12, m > 1 ? (double)i / (m - 1) : 0.0) : (i < m / 2 ? -100.0 + 1e-3 * i : 100.0 + 1e-3 * i);
    return k;
}

static int plain(const std::vector<double>& K, double X) { int s = 0; for (double k : K) s += k <= X ? 1 : 0; return s; }      // the number of knots <= X, counted

static long check_index(int m, int kind) {
    const std::vector<double> K = knots_of(m, kind);
    const int cells = fm_table_cells(m);
    std::vector<uint16_t> first((size_t)cells + 1);
    double scale = -1.0;
    table_index_build(K.data(), m, cells, &scale, first.data());
    if (!(scale >= 0.0) || first[0] != 0 || first[(size_t)cells] != (uint16_t)(m - 1)) die("the index's ends", m, kind);
    for (int c = 0; c < cells; ++c) if (first[(size_t)c] > first[(size_t)c + 1]) die("the index is not monotone", m, c);
    std::vector<uint16_t> wrong(first), zeros((size_t)cells + 1, 0), full((size_t)cells + 1, (uint16_t)m);
    for (int c = 0; c <= cells; ++c) wrong[(size_t)c] = (uint16_t)((first[(size_t)c] * 7 + c) % (m + 1));                      // any entries 0 … m
    long checked = 0, steps = 0;
    auto at = [&](double X) {
        const int want = X != X ? 0 : plain(K, X);
        if (fm_table_segment_plain(K.data(), m, X) != want) die("the plain search", m, kind);
        if (fm_table_segment(K.data(), m, first.data(), cells, scale, X) != want) die("the search by the index", m, kind);
        if (fm_table_segment(K.data(), m, wrong.data(), cells, scale, X) != want) die("the correction behind a wrong index", m, kind);
        if (fm_table_segment(K.data(), m, zeros.data(), cells, scale, X) != want || fm_table_segment(K.data(), m, full.data(), cells, scale, X) != want) die("the correction behind an empty index", m, kind);
        if (X == X && X >= K[0] && X < K[(size_t)m - 1]) {                      // the range of the cell holds s: the bisection alone finds it
            const int c = fm_table_cell(X, K[0], scale, cells);
            if (c < 0 || c >= cells || first[(size_t)c] > want || first[(size_t)c + 1] < want) die("the cell's range misses s", m, c);
            steps += first[(size_t)c + 1] - first[(size_t)c];
        }
        ++checked;
    };
    auto around = [&](double X) {
        at(X); at(std::nextafter(X, INFINITY)); at(std::nextafter(X, -INFINITY));
        const float f = (float)X;                                               // and as the kernel sees it: through fp32
        at((double)f); at((double)std::nextafterf(f, INFINITY)); at((double)std::nextafterf(f, -INFINITY));
    };
    for (double k : K) around(k);
    if (m > 1 && scale > 0.0)
        for (int c = 0; c <= cells; ++c) around(K[0] + (double)c / scale);      // the cell boundaries, as well as fp64 names them
    const double span = K[(size_t)m - 1] - K[0];
    for (double X : { K[0] - 1.0, K[0] - 1e30, K[(size_t)m - 1] + 1.0, 1e30, 0.0, -0.0, (double)INFINITY, -(double)INFINITY, (double)NAN,
                      (double)std::numeric_limits<float>::denorm_min(), -(double)std::numeric_limits<float>::denorm_min(), K[0] + 0.5 * span }) at(X);
    if (kind == 0 && m > 1 && steps > 2 * checked) die("uniform knots need more than one compare on average", m, steps);
    return checked;
}

// the kernel's loop: `blocks` workgroups of FM_TABLE_BLOCK lanes, a lane takes whole groups of four
static void model(const float* x, int64_t n, const std::vector<double>& K, const std::vector<double>& C, int T, uint32_t blocks, float* const* out) {
    const int m = (int)K.size(), cells = fm_table_cells(m);
    std::vector<uint16_t> first((size_t)cells + 1);
    double scale = 0.0;
    table_index_build(K.data(), m, cells, &scale, first.data());
    for (uint32_t block = 0; block < blocks; ++block)
        for (int lane = 0; lane < fm::FM_TABLE_BLOCK; ++lane)
            for (int64_t i4 = (int64_t)block * fm::FM_TABLE_BLOCK + lane; i4 * 4 < n; i4 += (int64_t)blocks * fm::FM_TABLE_BLOCK) {
                float xv[4], r[4][4];
                std::memcpy(xv, x + i4 * 4, 16);
                for (int j = 0; j < 4; ++j) {
                    const double X = (double)xv[j];
                    const int s = fm_table_segment(K.data(), m, first.data(), cells, scale, X);
                    const double a = K[(size_t)(s > 0 ? s - 1 : 0)];
                    for (int f = 0; f < T; ++f) r[f][j] = fm_table_value(C.data() + ((size_t)f * (size_t)(m + 1) + (size_t)s) * 4, X, a);
                }
                for (int f = 0; f < T; ++f) std::memcpy(out[f] + i4 * 4, r[f], 16);
            }
}

static void check_model(int64_t n, int m, int kind, int T, uint32_t blocks) {
    const std::vector<double> K = knots_of(m, kind);
    std::vector<double> V((size_t)m), C((size_t)T * (size_t)(m + 1) * 4);
    for (int f = 0; f < T; ++f) {
        for (int i = 0; i < m; ++i) V[(size_t)i] = std::sin(0.37 * i + f) + 0.01 * i;
        table_build(K.data(), V.data(), m, f % 4, (f / 2) % 2, f == 3 ? 1 : 0, C.data() + (size_t)f * (size_t)(m + 1) * 4);
    }
    const size_t cap = ((size_t)n * 4 + 255) / 256 * 256 / 4;                  // a vector's storage: a multiple of 256 bytes, and no more (ASan watches the end)
    std::vector<float> x(cap, std::numeric_limits<float>::quiet_NaN());
    uint64_t s = 88172645463325252ull + (uint64_t)n * 31 + (uint64_t)m;
    const double lo = K.front(), span = K.back() > K.front() ? K.back() - K.front() : 1.0;
    for (size_t p = 0; p < cap; ++p) {                                          // the padding holds values too: whatever lies there must be harmless
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        x[p] = p % 5 == 2 ? (float)K[(size_t)(s % (uint64_t)m)] : (float)(lo - 0.1 * span + 1.2 * span * ((double)(s >> 11) * 0x1.0p-53));
    }
    const float edge[] = { 0.0f, -0.0f, INFINITY, -INFINITY, NAN, std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max() };
    for (size_t e = 0; e < sizeof edge / sizeof *edge; ++e) { x[(e * 3) % (size_t)n] = edge[e]; x[(size_t)n - 1 - (e * 3) % (size_t)n] = edge[e]; }
    std::vector<std::vector<float>> got((size_t)T, std::vector<float>(cap, -7.0f)), want((size_t)T, std::vector<float>((size_t)n, -9.0f));
    float* g[4] = { nullptr, nullptr, nullptr, nullptr }; float* w[4] = { nullptr, nullptr, nullptr, nullptr };
    for (int f = 0; f < T; ++f) { g[f] = got[(size_t)f].data(); w[f] = want[(size_t)f].data(); }
    model(x.data(), n, K, C, T, blocks, g);
    table_apply_host(x.data(), n, K.data(), m, C.data(), T, w);
    for (int f = 0; f < T; ++f) {
        if (std::memcmp(g[f], w[f], (size_t)n * 4) != 0) die("the model differs from the definition", (long)n, m * 10 + f);
        for (size_t p = ((size_t)n + 3) / 4 * 4; p < cap; ++p) if (g[f][p] != -7.0f) die("the model wrote past the last group", (long)n, (long)p);
    }
}

int main() {
    long checked = 0;
    for (int kind = 0; kind < 3; ++kind)
        for (int m : { 1, 2, 3, 4, 5, 64, 65, 1023, 1024 }) checked += check_index(m, kind);
    const int64_t tile = fm::FM_TABLE_TILE;
    for (int64_t n : { (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)63, (int64_t)64, (int64_t)65, tile - 1, tile, tile + 1, 3 * tile + 3 })
        for (int kind = 0; kind < 3; ++kind) {
            check_model(n, 5, kind, 1, fm::table_blocks(n));
            check_model(n, 256, kind, 4, fm::table_blocks(n));
            check_model(n, 1024, kind, 1, fm::table_blocks(n));
        }
    check_model(3 * tile + 3, 65, 1, 2, 2);                                     // fewer workgroups than tiles: the grid-stride loop wraps
    check_model(7 * tile + 1, 1023, 2, 1, 3);
    if (fm::table_blocks((int64_t)fm::FM_TABLE_MAX_BLOCKS * tile) != (uint32_t)fm::FM_TABLE_MAX_BLOCKS || fm::table_blocks((int64_t)fm::FM_TABLE_MAX_BLOCKS * tile + 1) != (uint32_t)fm::FM_TABLE_MAX_BLOCKS
        || fm::table_blocks(tile + 1) != 2u || fm::table_blocks(1) != 1u) die("the grid", 0, 0);
    if (fm::table_lds_bytes(1024, 1, fm_table_cells(1024)) > 64 * 1024 || fm::table_lds_bytes(256, 4, fm_table_cells(256)) > 64 * 1024) die("the tables exceed 64 KiB of LDS", 0, 0);
    std::printf("table host ok: %ld searches\n", checked);
    return 0;
}
