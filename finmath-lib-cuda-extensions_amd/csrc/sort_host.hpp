// sort_host.hpp — the HOST half of the device sort: the DEFINITION of fmhip_argsort (fmhip_argsort_host), and the constants
// and chunk arithmetic that the kernels (sort_kernel.hip) and the engine (sort_engine.hpp) share.  No HIP in this header:
// tests/cpp/test_sort_host.cpp drives it, sanitized, on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "order_stats.hpp"

namespace fm {

constexpr int FM_SORT_BLOCK = 256;                 // four waves
constexpr int FM_SORT_ITEMS = 8;                   // elements per lane and tile
constexpr int FM_SORT_TILE = FM_SORT_BLOCK * FM_SORT_ITEMS;      // 2048 elements per workgroup and iteration
constexpr int FM_SORT_BINS = 256;                  // 8-bit digits: four passes over a 32-bit key
constexpr int FM_SORT_PASSES = 4;
constexpr int FM_SORT_MIN_CHUNK_TILES = 2;         // a workgroup's chunk is at least two tiles: half the rows in the table, and the running offsets from tile to tile are not a large-n path
constexpr int FM_SORT_MAX_BLOCKS = 1024;           // rows of the count table: four workgroups per CU
constexpr int FM_SORT_STREAM_MAX_BLOCKS = 8192;   // grid cap of the gather and the scores kernel (256 lanes, a quad each): above 4 · 256 · 8192 elements a lane takes a second quad
constexpr int FM_SORT_READBACK_CHUNK = 16 << 20;   // elements of the permutation per D2H copy of fmhip_argsort (64 MiB of pinned stage)
constexpr int FM_SORT_MAX_VALUES = 8;              // companion vectors of one fmhip_sort_by_key call
constexpr int64_t FM_SORT_MAX_N = 0x7fffffffLL;    // positions are uint32 and every position + one tile stays below 2^32

// The grid and the chunks are a function of n ALONE (as os_sum_blocks): workgroup w owns the tiles [w·chunk_tiles, (w+1)·chunk_tiles) ∩ [0, tiles)
// of the CURRENT order, in every pass and in both the count and the scatter kernel.
inline int64_t sort_tiles(int64_t n) { return (n + FM_SORT_TILE - 1) / FM_SORT_TILE; }
inline uint32_t sort_chunk_tiles(int64_t n)
{
    const int64_t per = (sort_tiles(n) + FM_SORT_MAX_BLOCKS - 1) / FM_SORT_MAX_BLOCKS;
    return (uint32_t)(per < FM_SORT_MIN_CHUNK_TILES ? FM_SORT_MIN_CHUNK_TILES : per);
}
inline uint32_t sort_blocks(int64_t n)
{
    const int64_t c = sort_chunk_tiles(n), b = (sort_tiles(n) + c - 1) / c;
    return (uint32_t)(b < 1 ? 1 : b);
}
inline bool sort_size_ok(int64_t n) { return n > 0 && n <= FM_SORT_MAX_N; }
// bytes of the count table [blocks][256] in the side-pass scratch
inline size_t sort_table_bytes(int64_t n) { return (size_t)sort_blocks(n) * FM_SORT_BINS * 4; }

// The definition: permutation[r] = the path at position r of the ascending sample — ascending in the key of §4.7 (os::key_of: the order of
// java.util.Arrays.sort(float[]), every NaN one key, the last), equal keys in ascending path order.  Four stable counting passes over 8-bit
// digits: what the device does, without its chunks.
inline void sort_argsort_host(const float* key, int64_t n, int64_t* permutation_out)
{
    if (!key || !permutation_out) throw std::invalid_argument("argsort: null pointer");
    if (!sort_size_ok(n)) throw std::invalid_argument("argsort of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    std::vector<uint32_t> k0((size_t)n), k1((size_t)n), i0((size_t)n), i1((size_t)n);
    for (int64_t p = 0; p < n; ++p) { k0[(size_t)p] = os::key_of(key[p]); i0[(size_t)p] = (uint32_t)p; }
    for (uint32_t shift = 0; shift < 32u; shift += 8u) {
        size_t at[FM_SORT_BINS + 1] = { 0 };
        for (int64_t p = 0; p < n; ++p) at[((k0[(size_t)p] >> shift) & 255u) + 1u]++;
        for (int d = 0; d < FM_SORT_BINS; ++d) at[d + 1] += at[d];
        for (int64_t p = 0; p < n; ++p) { const size_t to = at[(k0[(size_t)p] >> shift) & 255u]++; k1[to] = k0[(size_t)p]; i1[to] = i0[(size_t)p]; }
        k0.swap(k1); i0.swap(i1);
    }
    for (int64_t r = 0; r < n; ++r) permutation_out[r] = (int64_t)i0[(size_t)r];
}

// The offsets kernel's arithmetic: table[w][d] counts → first destinations, an exclusive scan in (digit, workgroup) order.
inline void sort_offsets_host(uint32_t* table, uint32_t blocks)
{
    uint32_t run = 0;
    for (int d = 0; d < FM_SORT_BINS; ++d)
        for (uint32_t w = 0; w < blocks; ++w) { uint32_t& t = table[(size_t)w * FM_SORT_BINS + d]; const uint32_t c = t; t = run; run += c; }
}

} // namespace fm
