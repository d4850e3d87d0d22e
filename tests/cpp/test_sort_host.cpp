// test_sort_host.cpp — the host half of the device sort (csrc/sort_host.hpp) on the CPU, built with -fsanitize=address,undefined by
// tests/test_sort_cpu.py: the definition of the order against std::stable_sort on the keys, the chunk arithmetic for n around every
// boundary (the chunks cover the tiles once, no workgroup is empty, the table has at most FM_SORT_MAX_BLOCKS rows, positions stay below
// 2^32), and a model of one pass as the kernels run it — count per chunk, offsets in (digit, workgroup) order, scatter chunk by chunk — whose
// four passes must give the definition's permutation.
#include "../../finmath-lib-cuda-extensions_amd/csrc/sort_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>

using namespace fm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static float from_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

static std::vector<float> sample(int64_t n, int family, std::mt19937& rng)
{
    std::vector<float> a((size_t)n);
    std::normal_distribution<float> normal(0.f, 1.f);
    for (int64_t p = 0; p < n; ++p) {
        float x;
        switch (family) {
        case 0: x = normal(rng); break;
        case 1: x = std::max(normal(rng) - 0.2f, 0.f) * ((rng() & 1u) ? 1.f : -1.f); break;        // half zeros of both signs
        case 2: x = 1.25f; break;
        case 3: x = from_bits((rng() & 1u) ? 0x7fc00000u | (rng() & 0xffu) : 0xffc00000u | (rng() & 0xffu)); break;      // all NaN
        default: {
            const uint32_t r = rng() % 16u;
            x = r == 0 ? std::numeric_limits<float>::infinity() : r == 1 ? -std::numeric_limits<float>::infinity()
              : r == 2 ? from_bits(0x7f800123u) : r == 3 ? from_bits(0xffc00001u) : r == 4 ? from_bits(rng() % 80u) : r == 5 ? -0.f : normal(rng);
        }
        }
        a[(size_t)p] = x;
    }
    return a;
}

static std::vector<int64_t> by_stable_sort(const std::vector<float>& a)
{
    std::vector<int64_t> perm(a.size());
    std::iota(perm.begin(), perm.end(), (int64_t)0);
    std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return os::key_of(a[(size_t)x]) < os::key_of(a[(size_t)y]); });
    return perm;
}

// the chunks of n: every tile in exactly one workgroup, none empty
static void check_chunks(int64_t n)
{
    const int64_t tiles = sort_tiles(n);
    const uint32_t chunk = sort_chunk_tiles(n), blocks = sort_blocks(n);
    CHECK(tiles >= 1 && tiles * FM_SORT_TILE >= n && (tiles - 1) * FM_SORT_TILE < n);
    CHECK(chunk >= (uint32_t)FM_SORT_MIN_CHUNK_TILES && blocks >= 1u && blocks <= (uint32_t)FM_SORT_MAX_BLOCKS);
    CHECK((int64_t)blocks * chunk >= tiles && ((int64_t)blocks - 1) * chunk < tiles);
    CHECK(((int64_t)blocks * chunk + 1) * FM_SORT_TILE <= (int64_t(1) << 32));      // a position plus one tile fits uint32
    CHECK(sort_table_bytes(n) == (size_t)blocks * 256u * 4u);
}

// one pass as the three kernels run it
static void model_pass(const std::vector<uint32_t>& k0, const std::vector<uint32_t>& i0, std::vector<uint32_t>& k1, std::vector<uint32_t>& i1, uint32_t shift)
{
    const int64_t n = (int64_t)k0.size(), tiles = sort_tiles(n);
    const uint32_t chunk = sort_chunk_tiles(n), blocks = sort_blocks(n);
    std::vector<uint32_t> table((size_t)blocks * FM_SORT_BINS, 0u);
    auto range = [&](uint32_t w, int64_t& from, int64_t& to) {
        const int64_t t0 = (int64_t)w * chunk, t1 = std::min<int64_t>(t0 + chunk, tiles);
        from = t0 * FM_SORT_TILE; to = std::min<int64_t>(t1 * FM_SORT_TILE, n);
    };
    int64_t covered = 0;
    for (uint32_t w = 0; w < blocks; ++w) {
        int64_t from, to; range(w, from, to);
        CHECK(from == covered && to > from);
        covered = to;
        for (int64_t p = from; p < to; ++p) table[(size_t)w * FM_SORT_BINS + ((k0[(size_t)p] >> shift) & 255u)]++;
    }
    CHECK(covered == n);
    sort_offsets_host(table.data(), blocks);
    std::vector<char> written((size_t)n, 0);
    for (uint32_t w = 0; w < blocks; ++w) {
        int64_t from, to; range(w, from, to);
        for (int64_t p = from; p < to; ++p) {
            const uint32_t at = table[(size_t)w * FM_SORT_BINS + ((k0[(size_t)p] >> shift) & 255u)]++;
            if (at >= (uint32_t)n || written[at]) { CHECK(!"a destination outside the sample or taken twice"); return; }
            written[at] = 1; k1[at] = k0[(size_t)p]; i1[at] = i0[(size_t)p];
        }
    }
}

static void check_sort(int64_t n, int family, std::mt19937& rng)
{
    const std::vector<float> a = sample(n, family, rng);
    std::vector<int64_t> got((size_t)n);
    sort_argsort_host(a.data(), n, got.data());
    CHECK(got == by_stable_sort(a));
    std::vector<uint32_t> k0((size_t)n), k1((size_t)n), i0((size_t)n), i1((size_t)n);
    for (int64_t p = 0; p < n; ++p) { k0[(size_t)p] = os::key_of(a[(size_t)p]); i0[(size_t)p] = (uint32_t)p; }
    for (uint32_t shift = 0; shift < 32u; shift += 8u) { model_pass(k0, i0, k1, i1, shift); k0.swap(k1); i0.swap(i1); }
    bool same = true;
    for (int64_t r = 0; r < n; ++r) same = same && (int64_t)i0[(size_t)r] == got[(size_t)r];
    CHECK(same);
}

int main()
{
    std::mt19937 rng(20240607u);
    const int64_t tile = FM_SORT_TILE, chunk = (int64_t)FM_SORT_MIN_CHUNK_TILES * FM_SORT_TILE, full = (int64_t)FM_SORT_MAX_BLOCKS * chunk;
    std::vector<int64_t> sizes = { 1, 2, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 100003 };
    for (int64_t n : sizes) { check_chunks(n); for (int family = 0; family < 5; ++family) check_sort(n, family, rng); }
    // where the chunks start to grow: the table is full
    for (int64_t n : { full - 1, full, full + 1 }) { check_chunks(n); check_sort(n, 4, rng); }
    CHECK(sort_blocks(full) == (uint32_t)FM_SORT_MAX_BLOCKS && sort_chunk_tiles(full) == (uint32_t)FM_SORT_MIN_CHUNK_TILES);
    CHECK(sort_chunk_tiles(full + 1) == (uint32_t)FM_SORT_MIN_CHUNK_TILES + 1u);
    // arithmetic only, up to the largest sample
    for (int64_t n : { full + tile, 3 * full - 1, 3 * full, 3 * full + 1, (int64_t(1) << 26), (int64_t(1) << 30) + 12345, FM_SORT_MAX_N - tile, FM_SORT_MAX_N - 1, FM_SORT_MAX_N }) check_chunks(n);
    CHECK(sort_size_ok(1) && sort_size_ok(FM_SORT_MAX_N) && !sort_size_ok(0) && !sort_size_ok(-1) && !sort_size_ok(FM_SORT_MAX_N + 1) && !sort_size_ok(int64_t(1) << 40));
    // refusals of the definition
    int refused = 0;
    float one = 1.f; int64_t out = 0;
    try { sort_argsort_host(nullptr, 1, &out); } catch (const std::invalid_argument&) { ++refused; }
    try { sort_argsort_host(&one, 1, nullptr); } catch (const std::invalid_argument&) { ++refused; }
    try { sort_argsort_host(&one, 0, &out); } catch (const std::invalid_argument&) { ++refused; }
    try { sort_argsort_host(&one, FM_SORT_MAX_N + 1, &out); } catch (const std::invalid_argument&) { ++refused; }
    CHECK(refused == 4);
    // offsets of a known table: two workgroups, digits 0 and 255 only
    std::vector<uint32_t> t(2 * 256, 0u);
    t[0] = 3; t[256] = 4; t[255] = 5; t[511] = 6;
    sort_offsets_host(t.data(), 2);
    CHECK(t[0] == 0 && t[256] == 3 && t[1] == 7 && t[255] == 7 && t[511] == 12);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("sort host ok\n");
    return 0;
}
