// group_kernel.h — host-callable launchers of the kernels of group_kernel.hip (engine side: group_engine.hpp): the keys of
// a reduce by key, and the segmented scan over the sorted (key, path) pairs that leaves count, sum, mean and variance per group.  The
// definition, and every function of it that the kernels call, is group_host.hpp's (no HIP in it: tests/cpp/test_group_host.cpp drives it on
// the CPU).  The order between the two is the radix sort's (launch_sort_pass, from_floats = 0); the chunks are the prefix passes'.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "group_host.hpp"
#include "sort_host.hpp"

namespace fm {

constexpr int FM_GROUP_BLOCK = 256;                 // lanes of a keys or a fill workgroup
constexpr int FM_GROUP_STREAM_MAX_BLOCKS = 8192;    // grid cap of the keys and the fill kernel: above it a lane takes a further element
constexpr int FM_GROUP_COUNTS = 0, FM_GROUP_S1 = 1, FM_GROUP_S1_S2 = 2;          // what a scan launch sums: nothing, the values, the values and their squares

// Device scratch of a scan (the side-pass scratch that need not be zero, behind the sort table), 256-byte aligned parts:
//   rows   [blocks] { the chunk's last run-prefix of S1 and S2, its last head position + 1 or 0 }     written by the totals kernel
//   bases  [blocks] { the base of chunk c for S1 and S2, the last head position + 1 before it }        written by the carry kernel
struct GroupRow { double s1, s2; uint32_t head, pad; };
constexpr size_t group_rows_bytes(int64_t n) { return prefix_up256((size_t)prefix_blocks(n) * sizeof(GroupRow)); }
constexpr size_t group_scan_scratch_bytes(int64_t n) { return 2 * group_rows_bytes(n); }
inline size_t group_table_bytes(int64_t n) { return prefix_up256(sort_table_bytes(n)); }
inline size_t group_scratch_bytes(int64_t n) { return group_table_bytes(n) + group_scan_scratch_bytes(n); }

struct DevGroupKeysArgs {
    uint32_t  n, m;            // elements of the index, groups
    uint64_t  index;           // n floats
    uint64_t  key_out, idx_out;        // n uint32 each: group_key(index[j], m) and j
};
struct DevGroupScanArgs {
    uint32_t  n, m;
    uint32_t  chunk_tiles;     // prefix_chunk_tiles(n)
    uint32_t  mode;            // FM_GROUP_COUNTS, FM_GROUP_S1, FM_GROUP_S1_S2
    uint32_t  mask;            // the outputs of `values`: FM_BLOCK_SUM | MEAN | VARIANCE; 0 with FM_GROUP_COUNTS
    uint32_t  pad;
    uint64_t  key, perm;       // n uint32 each: the sorted keys and the path of every sorted position
    uint64_t  values;          // n floats, or 0 with FM_GROUP_COUNTS
    uint64_t  counts_out;      // m floats, or 0
    uint64_t  outs[fmhost::FM_BLOCK_MAX_OUTPUTS];   // m floats each, the mask's bits in ascending order
    char*     scratch;         // device: group_scan_scratch_bytes(n)
    uint64_t* ungrouped_host;  // pinned, or null: the number of ungrouped elements — written by the lane that holds the head of the last run (key m), or 0 by the one whose tail at n - 1 has a key below m
};
inline bool group_keys_shape_ok(const DevGroupKeysArgs& a)
{
    return a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.m > 0 && a.m <= (uint32_t)FM_GROUP_MAX_M && a.index && a.key_out && a.idx_out;
}
inline bool group_scan_shape_ok(const DevGroupScanArgs& a)
{
    if (!(a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.m > 0 && a.m <= (uint32_t)FM_GROUP_MAX_M && a.chunk_tiles == prefix_chunk_tiles(a.n))) return false;
    if (!(a.key && a.perm && a.scratch) || a.mode > (uint32_t)FM_GROUP_S1_S2 || (a.mask & ~FM_GROUP_MASK_ALL) != 0u) return false;
    if (a.mode == (uint32_t)FM_GROUP_COUNTS) return a.mask == 0u && !a.values && (a.counts_out || a.ungrouped_host);
    if (!a.values || a.mask == 0u) return false;
    if (((a.mask & (uint32_t)fmhost::FM_BLOCK_VARIANCE) != 0u) != (a.mode == (uint32_t)FM_GROUP_S1_S2)) return false;
    for (int j = 0; j < fmhost::fm_block_outputs(a.mask); ++j) if (!a.outs[j]) return false;
    return true;
}
#if defined(__HIP__)
#define FM_GROUP_ARGS_HD __host__ __device__
#else
#define FM_GROUP_ARGS_HD
#endif
FM_GROUP_ARGS_HD inline GroupRow* group_rows(const DevGroupScanArgs& a) { return reinterpret_cast<GroupRow*>(a.scratch); }
FM_GROUP_ARGS_HD inline GroupRow* group_bases(const DevGroupScanArgs& a) { return reinterpret_cast<GroupRow*>(a.scratch + group_rows_bytes(a.n)); }

// key_out[j] = group_key(index[j], m), idx_out[j] = j
hipError_t launch_group_keys(const DevGroupKeysArgs& a, hipStream_t st);
// fill → totals → carry → apply over the sorted pairs, chained on `st`: count and the masked outputs of ONE value vector at [key]
hipError_t launch_group_scan(const DevGroupScanArgs& a, hipStream_t st);

} // namespace fm
