// block_order_kernel.h — host-callable launcher of the kernels of block_order_kernel.hip (engine side:
// block_order_engine.hpp; definition: host/block_order.hpp): selected ranks and range means of the consecutive blocks of up to four vectors
// as new vectors of one element per block, or every block sorted in place of a copy.  The regimes and the grid are functions of `block` and
// the sizes alone and live here (no HIP in them: tests/nulldev/null_block_order.cpp uses them on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/block_order.hpp"

namespace fm {

constexpr int FM_ORDER_SMALL_BLOCK = 256;              // small regime: lanes of a workgroup, four waves with tasks of their own
constexpr int FM_ORDER_SMALL_WAVES = FM_ORDER_SMALL_BLOCK / 64;
constexpr int FM_ORDER_SMALL_MAX_BLOCKS = 4096;        // its grid's cap: beyond it the wave-stride loop over the tasks wraps
constexpr int64_t FM_ORDER_SMALL = 64;                 // block <= 64: 64 / fm_block_width(block) blocks share a wave, keys in registers
                                                       // above: one workgroup per block, keys padded to a power of two P in registers and LDS
constexpr int64_t FM_ORDER_SWEEP = 1 << 20;            // medium regime: padded elements of one sweep of the grid — its cap is FM_ORDER_SWEEP / P
constexpr int64_t FM_ORDER_MIN_GROUPS = 256, FM_ORDER_MAX_GROUPS = 8192;

struct DevBlockOrderArgs {
    int64_t   n, block;                                // n = m·block, block <= FM_BLOCK_ORDER_MAX
    uint32_t  n_vectors, n_ranks, n_ranges, sort;      // sort != 0: the block sort into out[slot][0] (n elements), no selector
    uint32_t  ranks[fmhost::FM_BLOCK_ORDER_MAX_RANKS];
    uint32_t  range_from[fmhost::FM_BLOCK_ORDER_MAX_RANGES], range_to[fmhost::FM_BLOCK_ORDER_MAX_RANGES];
    uint64_t  v[fmhost::FM_BLOCK_ORDER_MAX_VECTORS];   // addresses (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_BLOCK_ORDER_MAX_VECTORS][fmhost::FM_BLOCK_ORDER_MAX_OUTPUTS];     // [vector][j]: ranks first, then ranges; n / block floats each
};

inline bool order_is_small(int64_t block) { return block <= FM_ORDER_SMALL; }
// medium regime: the power of two >= block, 128 … 4096
inline int order_padded(int64_t block) { int p = 128; while (p < block) p <<= 1; return p; }
// lanes of its workgroup: at most 4 keys per lane above P = 1024, where the grid's cap leaves one or two workgroups per CU
constexpr int order_lanes(int padded) { return padded < 256 ? 128 : padded <= 1024 ? 256 : 1024; }
inline uint32_t order_grid(int64_t n, int64_t block)
{
    const int64_t m = n / block;
    if (order_is_small(block)) {
        const int64_t per = 64 / fmhost::fm_block_width(block), tasks = (m + per - 1) / per, b = (tasks + FM_ORDER_SMALL_WAVES - 1) / FM_ORDER_SMALL_WAVES;
        return (uint32_t)(b > FM_ORDER_SMALL_MAX_BLOCKS ? FM_ORDER_SMALL_MAX_BLOCKS : b);
    }
    int64_t cap = FM_ORDER_SWEEP / order_padded(block);
    cap = cap < FM_ORDER_MIN_GROUPS ? FM_ORDER_MIN_GROUPS : cap > FM_ORDER_MAX_GROUPS ? FM_ORDER_MAX_GROUPS : cap;
    return (uint32_t)(m < cap ? m : cap);
}
inline bool block_order_shape_ok(const DevBlockOrderArgs& a)
{
    if (a.n < 1 || a.n > fmhost::FM_BLOCK_MAX_N || a.block < 1 || a.block > fmhost::FM_BLOCK_ORDER_MAX || a.n % a.block != 0) return false;
    if (a.n_vectors < 1 || a.n_vectors > (uint32_t)fmhost::FM_BLOCK_ORDER_MAX_VECTORS) return false;
    if (a.n_ranks > (uint32_t)fmhost::FM_BLOCK_ORDER_MAX_RANKS || a.n_ranges > (uint32_t)fmhost::FM_BLOCK_ORDER_MAX_RANGES) return false;
    if (a.sort ? (a.n_ranks + a.n_ranges != 0u) : (a.n_ranks + a.n_ranges == 0u)) return false;
    for (uint32_t j = 0; j < a.n_ranks; ++j) if ((int64_t)a.ranks[j] >= a.block) return false;
    for (uint32_t j = 0; j < a.n_ranges; ++j) if (a.range_from[j] > a.range_to[j] || (int64_t)a.range_to[j] >= a.block) return false;
    const uint32_t n_out = a.sort ? 1u : a.n_ranks + a.n_ranges;
    for (uint32_t i = 0; i < a.n_vectors; ++i) {
        if (!a.v[i]) return false;
        for (uint32_t j = 0; j < n_out; ++j) if (!a.out[i][j] || a.out[i][j] == a.v[i]) return false;
    }
    return true;
}

// ONE launch: every vector of the call (blockIdx.y), every block
hipError_t launch_block_order(const DevBlockOrderArgs& a, hipStream_t st);

} // namespace fm
