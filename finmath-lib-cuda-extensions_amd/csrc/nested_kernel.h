// nested_kernel.h — host-callable launchers of the kernels of nested_kernel.hip (engine side: nested_engine.hpp;
// definition: host/block_moments.hpp): the moments of consecutive blocks of up to four vectors as new vectors of one element per block, and
// the repeat that nested simulation starts from.  The regimes, the grid and the layout of the scratch are functions of `block` and the
// sizes alone and live here (no HIP in them: tests/nulldev/null_nested.cpp uses them on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/block_moments.hpp"

namespace fm {

constexpr int FM_NESTED_BLOCK = 256;                   // lanes of a workgroup: four waves, each with tasks of its own
constexpr int FM_NESTED_WAVES = FM_NESTED_BLOCK / 64;
constexpr int FM_NESTED_MAX_BLOCKS = 4096;             // the grid's cap: beyond it the wave-stride loop over the tasks wraps
constexpr int64_t FM_NESTED_SMALL = 64;                // block <= 64: several blocks share a wave (64 / fm_block_width(block) of them)
                                                       // 64 < block <= FM_BLOCK_SEGMENT: one wave per block;  above: one wave per segment and a second stage

struct DevBlockMomentsArgs {
    int64_t   n, block;                                // n = m·block
    uint32_t  n_vectors, mask;                         // 1 … 4; FM_BLOCK_* bits
    uint64_t  v[fmhost::FM_BLOCK_MAX_VECTORS];         // addresses (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_BLOCK_MAX_VECTORS][fmhost::FM_BLOCK_MAX_OUTPUTS];      // [vector][j]: one per set bit of the mask, in bit order; n / block floats each
    double*   partials;                                // device scratch of block_partials_bytes (large blocks only): [vector][block][segment] { s1, s2 }
};
struct DevRepeatArgs {
    int64_t   n, each, times;                          // out[(t·n + p)·each + e] = v[p]; n·each·times <= 2^31 − 1
    uint64_t  v, out;
};

inline bool block_is_small(int64_t block) { return block <= FM_NESTED_SMALL; }
inline bool block_is_large(int64_t block) { return block > fmhost::FM_BLOCK_SEGMENT; }
// tasks of one vector: a wave's iteration
inline int64_t block_tasks(int64_t n, int64_t block)
{
    const int64_t m = n / block;
    if (block_is_small(block)) { const int64_t per = 64 / fmhost::fm_block_width(block); return (m + per - 1) / per; }
    return m * fmhost::fm_block_segments(block);
}
inline uint32_t nested_grid(int64_t tasks)
{
    const int64_t b = (tasks + FM_NESTED_WAVES - 1) / FM_NESTED_WAVES;
    return (uint32_t)(b < 1 ? 1 : b > FM_NESTED_MAX_BLOCKS ? FM_NESTED_MAX_BLOCKS : b);
}
inline size_t block_partials_bytes(int64_t n, int64_t block, int n_vectors)
{
    return block_is_large(block) ? (size_t)n_vectors * (size_t)(n / block) * (size_t)fmhost::fm_block_segments(block) * 16 : 0;
}
inline bool block_moments_shape_ok(const DevBlockMomentsArgs& a)
{
    if (a.n < 1 || a.n > fmhost::FM_BLOCK_MAX_N || a.block < 1 || a.n % a.block != 0) return false;
    if (a.n_vectors < 1 || a.n_vectors > (uint32_t)fmhost::FM_BLOCK_MAX_VECTORS || a.mask < 1 || a.mask > (uint32_t)fmhost::FM_BLOCK_ALL) return false;
    for (uint32_t i = 0; i < a.n_vectors; ++i) {
        if (!a.v[i]) return false;
        for (int j = 0; j < fmhost::fm_block_outputs(a.mask); ++j) if (!a.out[i][j] || a.out[i][j] == a.v[i]) return false;
    }
    return !block_is_large(a.block) || a.partials != nullptr;
}
inline bool repeat_shape_ok(const DevRepeatArgs& a)
{
    if (a.n < 1 || a.each < 1 || a.times < 1 || !a.v || !a.out || a.v == a.out) return false;
    return a.each <= fmhost::FM_BLOCK_MAX_N / a.n && a.times <= fmhost::FM_BLOCK_MAX_N / (a.n * a.each);
}

// the block kernel, and for large blocks the combine of the segments' partials behind it, chained on `st`
hipError_t launch_block_moments(const DevBlockMomentsArgs& a, hipStream_t st);
hipError_t launch_repeat(const DevRepeatArgs& a, hipStream_t st);

} // namespace fm
