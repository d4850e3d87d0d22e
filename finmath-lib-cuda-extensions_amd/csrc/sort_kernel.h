// sort_kernel.h — host-callable launchers of the kernels of sort_kernel.hip (engine side: sort_engine.hpp): a stable
// least-significant-digit radix sort of (key, path index) pairs by the 32-bit key of §4.7, and the three kernels that turn the permutation
// into results — gather, scatter-score, read-elements.  The constants and the chunk arithmetic are sort_host.hpp's (no HIP in it:
// tests/cpp/test_sort_host.cpp drives them on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "sort_host.hpp"

namespace fm {

// One pass: digit = (key >> shift) & 255.  The first pass reads the float vector itself (key = os_key(x), index = position); the others read
// the pair the pass before wrote.  The last pass writes no keys: nobody reads them.
struct DevSortPassArgs {
    uint32_t  n;
    uint32_t  chunk_tiles;     // sort_chunk_tiles(n); the grid is sort_blocks(n)
    uint32_t  shift;           // 0, 8, 16, 24
    uint32_t  from_floats;     // 1: src_key is the float vector, src_idx unused
    uint32_t  write_keys;
    uint64_t  src_key, src_idx;        // addresses, 256-byte aligned
    uint64_t  dst_key, dst_idx;
    uint32_t* table;           // [blocks][256]: counts after the count kernel, first destinations after the offsets kernel
};
inline bool sort_pass_shape_ok(const DevSortPassArgs& a)
{
    return a.n > 0 && a.n <= (uint32_t)FM_SORT_MAX_N && a.chunk_tiles == sort_chunk_tiles(a.n) && a.shift <= 24u && (a.shift & 7u) == 0u
        && a.src_key && (a.from_floats || a.src_idx) && a.dst_idx && (!a.write_keys || a.dst_key) && a.table
        && a.src_key != a.dst_key && a.src_idx != a.dst_idx;
}
// count → offsets → scatter, chained on `st`
hipError_t launch_sort_pass(const DevSortPassArgs& a, hipStream_t st);

// out[k][r] = src[k][perm[r]] for `count` vectors, by bit copy
struct DevSortGatherArgs {
    uint32_t  n, count;        // count <= 1 + FM_SORT_MAX_VALUES
    uint64_t  perm;            // address of the uint32 permutation
    uint64_t  src[1 + FM_SORT_MAX_VALUES], dst[1 + FM_SORT_MAX_VALUES];
};
hipError_t launch_sort_gather(const DevSortGatherArgs& a, hipStream_t st);
// out[perm[r]] = (float)((r + 0.5) / n), the quotient in fp64
hipError_t launch_sort_scores(uint64_t perm, uint64_t out, uint32_t n, hipStream_t st);
// out[j] = (double)v[pos[j]] into pinned memory; pos: device, [count], every entry below n (the host has checked)
hipError_t launch_sort_read_elements(uint64_t v, const uint32_t* pos, uint32_t count, double* out_host, hipStream_t st);
// the end of a chain: *done_flag = done_value behind everything the stream has run
hipError_t launch_sort_done(uint64_t* done_flag, uint64_t done_value, hipStream_t st);

} // namespace fm
