// select_kernel.h — host-callable launchers of the kernels of select_kernel.hip (engine side: select_engine.hpp): the
// count of the selected elements of a mask, the compress and the expand that follow it, and the gather by a caller's index.  The
// definition, and every function of it that the kernels call, is select_host.hpp's (no HIP in it: tests/cpp/test_select_host.cpp drives
// it on the CPU).  The chunks are the prefix passes' (prefix_host.hpp): workgroup w owns the tiles of chunk w.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "select_host.hpp"

namespace fm {

constexpr int FM_SELECT_BLOCK = 256;                // lanes of a gather workgroup
constexpr int FM_SELECT_ITEMS = 4;                  // outputs per lane, FM_SELECT_BLOCK apart: every store of a wave is 256 contiguous bytes
constexpr int FM_SELECT_TILE = FM_SELECT_BLOCK * FM_SELECT_ITEMS;

// Device scratch of a compress or an expand (the side-pass scratch that need not be zero), 256-byte aligned parts:
//   counts  [blocks]      the selected elements of chunk c                                  written by the count kernel
//   bases   [blocks + 1]  the selected elements before chunk c, then the count of the mask   written by the carry kernel
constexpr size_t select_counts_bytes(int64_t n) { return prefix_up256((size_t)prefix_blocks(n) * 4); }
constexpr size_t select_scratch_bytes(int64_t n) { return select_counts_bytes(n) + prefix_up256(((size_t)prefix_blocks(n) + 1) * 4); }

struct DevCompressArgs {
    uint32_t  n;               // elements of the mask
    uint32_t  count;           // phase 2: the count that the host read — the size of every compressed vector
    uint32_t  chunk_tiles;     // prefix_chunk_tiles(n)
    uint32_t  n_values;        // 0 … FM_SELECT_MAX_VALUES
    float     fill;            // expand
    uint32_t  pad;
    uint64_t  mask;            // n floats
    uint64_t  values[FM_SELECT_MAX_VALUES], values_out[FM_SELECT_MAX_VALUES];       // compress: n resp. count floats; expand: count resp. n
    uint64_t  positions_out;   // compress: count floats, or 0
    char*     scratch;         // device: select_scratch_bytes(n)
    uint64_t* count_host;      // pinned: the count of the mask (phase 1)
};
struct DevIndexGatherArgs {
    uint32_t  n, m;            // elements of the values, of the index and the outputs
    uint32_t  n_values;        // 1 … FM_SELECT_MAX_VALUES
    uint32_t  pad;
    uint64_t  index;           // m floats
    uint64_t  values[FM_SELECT_MAX_VALUES], values_out[FM_SELECT_MAX_VALUES];       // n resp. m floats
};
inline bool select_count_shape_ok(const DevCompressArgs& a)
{
    return a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.chunk_tiles == prefix_chunk_tiles(a.n) && a.mask && a.scratch && a.count_host;
}
inline bool select_shape_ok(const DevCompressArgs& a, bool expand)
{
    if (!(a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.chunk_tiles == prefix_chunk_tiles(a.n) && a.mask && a.scratch)) return false;
    if (!(a.count > 0 && a.count <= a.n && a.n_values <= (uint32_t)FM_SELECT_MAX_VALUES)) return false;
    if (expand ? a.n_values == 0u || a.positions_out != 0 : a.n_values == 0u && !a.positions_out) return false;
    if (a.positions_out && a.n > (uint32_t)FM_SELECT_MAX_POSITION_N) return false;
    for (uint32_t i = 0; i < a.n_values; ++i) if (!a.values[i] || !a.values_out[i]) return false;
    return true;
}
inline bool gather_shape_ok(const DevIndexGatherArgs& a)
{
    if (!(a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.m > 0 && a.m <= (uint32_t)FM_PREFIX_MAX_N && a.n_values > 0 && a.n_values <= (uint32_t)FM_SELECT_MAX_VALUES && a.index)) return false;
    for (uint32_t i = 0; i < a.n_values; ++i) if (!a.values[i] || !a.values_out[i]) return false;
    return true;
}
#if defined(__HIP__)
#define FM_SELECT_ARGS_HD __host__ __device__
#else
#define FM_SELECT_ARGS_HD
#endif
FM_SELECT_ARGS_HD inline uint32_t* select_counts(const DevCompressArgs& a) { return reinterpret_cast<uint32_t*>(a.scratch); }
FM_SELECT_ARGS_HD inline uint32_t* select_bases(const DevCompressArgs& a) { return reinterpret_cast<uint32_t*>(a.scratch + select_counts_bytes(a.n)); }

// phase 1: counts → carry (the bases into the scratch, the count into pinned memory).  Chained on `st`.
hipError_t launch_select_count(const DevCompressArgs& a, hipStream_t st);
// phase 2, behind phase 1 of the same mask on the same scratch: the scatter resp. the expansion
hipError_t launch_select_compress(const DevCompressArgs& a, hipStream_t st);
hipError_t launch_select_expand(const DevCompressArgs& a, hipStream_t st);
hipError_t launch_select_gather(const DevIndexGatherArgs& a, hipStream_t st);

} // namespace fm
