// prefix_host.hpp — the HOST half of the device prefix sums: the DEFINITION of P[r] (fmhip_prefix_sums_host), and the
// constants and chunk arithmetic that the kernels (prefix_kernel.hip) and the engine (prefix_engine.hpp) share.  No HIP in this header:
// tests/cpp/test_prefix_host.cpp drives it, sanitized, on the CPU.
//
// THE TREE.  P[r] is the fp64 sum of (double)v[0..r] in ONE association, a function of n and r alone.  The sample is cut into nested units:
//   level 0  an element                                level 4  a tile  = 4 waves   (2048 elements)
//   level 1  a lane  = 8 consecutive elements          level 5  a chunk = prefix_chunk_tiles(n) consecutive tiles
//   level 2  a group = 8 lanes     (64 elements)       level 6  the sample = prefix_blocks(n) chunks
//   level 3  a wave  = 8 groups   (512 elements)
// and the prefixes of a unit are made from those of its subunits by ONE rule: the first subunit's prefixes are taken as they are (they are
// not added to 0: a leading -0.0 stays -0.0); subunit j's BASE is the last prefix of subunit j - 1 of that same level, and every prefix of
// subunit j is fl(base + its prefix inside the subunit).  A subunit cut short by n is scanned as far as it goes.
// fl(a + b) is monotone in b and a subunit's last prefix is the next one's base, bit for bit — so for input without negative elements or
// NaNs P is non-decreasing (a cumulative weight is a CDF), which a Kogge–Stone association does not give.  And a unit's largest prefix is
// fl(base + its largest prefix inside), which is what lets a search find its chunk from one number per chunk.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace fm {

constexpr int FM_PREFIX_ITEMS = 8;                  // elements per lane: two 16-byte loads
constexpr int FM_PREFIX_GROUP = 8;                  // lanes per group
constexpr int FM_PREFIX_GROUPS = 8;                 // groups per wave
constexpr int FM_PREFIX_WAVES = 4;                  // waves per tile
constexpr int FM_PREFIX_BLOCK = 64 * FM_PREFIX_WAVES;
constexpr int FM_PREFIX_WAVE_ELEMS = 64 * FM_PREFIX_ITEMS;                   // 512
constexpr int FM_PREFIX_TILE = FM_PREFIX_BLOCK * FM_PREFIX_ITEMS;            // 2048 elements per workgroup and iteration
constexpr int FM_PREFIX_MIN_CHUNK_TILES = 2;        // a chunk is at least two tiles: the tile-to-tile carry is not a large-n path
constexpr int FM_PREFIX_MAX_BLOCKS = 1024;          // rows of the totals table: four workgroups per CU
constexpr int FM_PREFIX_MAX_QUERIES = 4096;         // positions of one fmhip_prefix_sums_at, thresholds of one fmhip_prefix_search
constexpr int FM_PREFIX_CARRY_BLOCK = 1024;         // lanes of the one workgroup of the carry kernel
constexpr int64_t FM_PREFIX_MAX_N = 0x7fffffffLL;   // positions are uint32 and every position + one tile stays below 2^32
constexpr int FM_PREFIX_SUM = 0, FM_PREFIX_MEAN = 1;                         // FMHIP_PREFIX_SUM, FMHIP_PREFIX_MEAN
static_assert(FM_PREFIX_GROUP * FM_PREFIX_GROUPS == 64, "a wave is 64 lanes");

// (constexpr: the kernels call them too)
// The grid and the chunks are a function of n ALONE: workgroup w owns the tiles [w·chunk_tiles, (w+1)·chunk_tiles) ∩ [0, tiles).
constexpr int64_t prefix_tiles(int64_t n) { return (n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE; }
constexpr uint32_t prefix_chunk_tiles(int64_t n)
{
    const int64_t per = (prefix_tiles(n) + FM_PREFIX_MAX_BLOCKS - 1) / FM_PREFIX_MAX_BLOCKS;
    return (uint32_t)(per < FM_PREFIX_MIN_CHUNK_TILES ? FM_PREFIX_MIN_CHUNK_TILES : per);
}
constexpr int64_t prefix_chunk_elems(int64_t n) { return (int64_t)prefix_chunk_tiles(n) * FM_PREFIX_TILE; }
constexpr uint32_t prefix_blocks(int64_t n)
{
    const int64_t c = prefix_chunk_tiles(n), b = (prefix_tiles(n) + c - 1) / c;
    return (uint32_t)(b < 1 ? 1 : b);
}
constexpr bool prefix_size_ok(int64_t n) { return n > 0 && n <= FM_PREFIX_MAX_N; }
// The longest chain of additions behind any P[r]: 7 along a lane, 7 over the lanes of a group, 7 over the groups of a wave, 3 over the
// waves of a tile, then one per further tile of the chunk and one per further chunk.  |P[r] - exact| <= (prefix_chain(n) + 1)·2^-53·Σ_{i<=r}|v[i]|.
constexpr int prefix_chain(int64_t n)
{
    return (FM_PREFIX_ITEMS - 1) + (FM_PREFIX_GROUP - 1) + (FM_PREFIX_GROUPS - 1) + (FM_PREFIX_WAVES - 1) + ((int)prefix_chunk_tiles(n) - 1) + ((int)prefix_blocks(n) - 1);
}

// Device scratch of a call (the side-pass scratch that need not be zero), 256-byte aligned parts:
//   rows     [blocks] { total, largest prefix inside the chunk }     written by the totals kernel
//   bases    [blocks] the base of chunk c (entry 0 is not used: the first chunk takes none), then the total P[n-1]
//   queries  [count]  8 bytes each: a position (uint64) or a threshold (double), copied in from the host
//   located  [count]  { the threshold in force, the chunk } per query, written by the carry kernel
struct PrefixRow { double total, largest; };
struct PrefixLocated { double threshold; uint32_t chunk, pad; };
constexpr size_t prefix_up256(size_t b) { return (b + 255) & ~size_t(255); }
constexpr size_t prefix_rows_bytes(int64_t n) { return prefix_up256((size_t)prefix_blocks(n) * sizeof(PrefixRow)); }
constexpr size_t prefix_bases_bytes(int64_t n) { return prefix_up256(((size_t)prefix_blocks(n) + 1) * 8); }
constexpr size_t prefix_queries_bytes(int count) { return prefix_up256((size_t)count * 8); }
constexpr size_t prefix_located_bytes(int count) { return prefix_up256((size_t)count * sizeof(PrefixLocated)); }
constexpr size_t prefix_scratch_bytes(int64_t n, int count) { return prefix_rows_bytes(n) + prefix_bases_bytes(n) + prefix_queries_bytes(count) + prefix_located_bytes(count); }

// The prefixes of ONE unit of `level` (1 … 6) that holds m elements, into p[0..m): the rule above.
inline void prefix_unit_host(const float* v, int64_t m, double* p, int level, int64_t chunk_elems)
{
    if (level == 1) {
        double run = (double)v[0];
        p[0] = run;
        for (int64_t i = 1; i < m; ++i) { run = run + (double)v[i]; p[i] = run; }
        return;
    }
    const int64_t sub = level == 2 ? FM_PREFIX_ITEMS : level == 3 ? FM_PREFIX_ITEMS * FM_PREFIX_GROUP : level == 4 ? FM_PREFIX_WAVE_ELEMS : level == 5 ? FM_PREFIX_TILE : chunk_elems;
    double base = 0.0;
    for (int64_t off = 0; off < m; off += sub) {
        const int64_t cnt = m - off < sub ? m - off : sub;
        prefix_unit_host(v + off, cnt, p + off, level - 1, chunk_elems);
        if (off > 0) for (int64_t i = 0; i < cnt; ++i) p[off + i] = base + p[off + i];
        base = p[off + cnt - 1];
    }
}

// The definition: prefix_out[r] = P[r], r = 0 … n - 1.
inline void prefix_sums_host(const float* v, int64_t n, double* prefix_out)
{
    if (!v || !prefix_out) throw std::invalid_argument("prefix sums: null pointer");
    if (!prefix_size_ok(n)) throw std::invalid_argument("prefix sums of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    prefix_unit_host(v, n, prefix_out, 6, prefix_chunk_elems(n));
}

// out[r] of fmhip_prefix_sums from P[r]
inline float prefix_out_host(double p, int64_t r, int mode) { return mode == FM_PREFIX_MEAN ? (float)(p / (double)(r + 1)) : (float)p; }

// The smallest r with P[r] >= t, or n: the definition of fmhip_prefix_search over the definition's prefixes (a NaN never qualifies).
inline int64_t prefix_search_host(const double* prefix, int64_t n, double t)
{
    for (int64_t r = 0; r < n; ++r) if (prefix[r] >= t) return r;
    return n;
}

} // namespace fm
