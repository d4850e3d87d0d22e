// kernels.h — host-callable launchers of the gfx950 kernels in kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "fm_program.h"

namespace fm {

struct DevBmArgs {
    float*       slab;           // n_streams vectors, `stride_floats` apart (stride is a multiple of 64 floats)
    const float* sqrt_dt;        // [n_streams]  (float)sqrt(dt[step of the stream]), one entry per local stream
    int64_t      stride_floats;
    int64_t      n_paths;        // paths held by this process
    int64_t      path_offset;    // global index of local path 0 (path sharding over GPUs)
    uint32_t     key0, key1;     // lo32(seed), hi32(seed)
    uint32_t     n_factors;
    uint32_t     stream0;        // global stream index (step*n_factors+factor) of local stream 0
};

hipError_t launch_program(const DevProgramArgs& a, const uint64_t* rows, double* partials,
                          uint32_t blocks_per_row, uint32_t batch, hipStream_t st);
hipError_t launch_bm(const DevBmArgs& a, uint32_t n_streams, hipStream_t st);
hipError_t launch_fill(float* p, float v, int64_t n_padded, hipStream_t st);
hipError_t preload_kernels();        // makes the device code of every kernel above resident (the runtime would load it at first launch)

// {Σ, Σ², min, max} blocks of 32 bytes collected from wherever the launches that took them left them (slots of the pinned moments arena,
// mapped into the device's address space) into one contiguous device buffer — the send buffer of an RCCL exchange.
constexpr int FM_GATHER_MAX = 384;                 // sources per launch: they travel in the kernel arguments (3 KB of the 4 KB segment)
struct DevGatherArgs { uint32_t count; uint32_t pad; uint64_t src[FM_GATHER_MAX]; };
hipError_t launch_gather_moments(const DevGatherArgs& a, double* out, hipStream_t st);
// gathered[world][count][4] → out[count][4]: the shards' moments combined in shard order by fmhip_expectation_combine's rule (on the device that holds them)
hipError_t launch_combine_moments(const double* gathered, uint32_t world, uint32_t count, double* out, hipStream_t st);

// ---- order statistics (order_stats_engine.hpp): radix select by host-stepped digit histograms, the fp64 sum of the elements
// strictly between two keys, and the counts of the elements per interval of a sorted list of bounds.  Every launch leaves its integers
// (or sums) in pinned host memory and raises a flag behind them; the device-side scratch it counts in is zero again when it ends.
constexpr int FM_OS_BINS = 256;                    // 8-bit digits: four passes over a 32-bit key
constexpr int FM_OS_MAX_SLOTS = 8;                 // distinct prefixes per vector and launch (8 KB of LDS histograms)
constexpr int FM_OS_TILE = 4096;                   // elements per workgroup and iteration: 256 lanes x 4 x 16 bytes
constexpr int FM_OS_MAX_BOUNDS = 4096;             // bounds per counting launch (32 KB of LDS)
struct DevOsCommon {
    uint32_t* counters;        // [batch + 1] arrival counters: one per vector, one for the launch
    uint64_t* done_flag;       // pinned; receives done_value when everything below is in host memory
    uint64_t  done_value;
    int64_t   n;
    uint32_t  tiles;           // ceil(n / FM_OS_TILE)
    uint32_t  use_inline;      // one vector: its address (and slots / keys) travel in the arguments
    uint64_t  vec0;
};
struct DevSelectArgs {
    DevOsCommon c;
    uint32_t* hist_dev;        // [batch][S][256]
    uint32_t* hist_host;       // pinned, same shape
    uint32_t  S;               // slots per vector in the tables
    uint32_t  shift;           // digit = (key >> shift) & 255; an element belongs to a slot when its key agrees with the slot's prefix above the digit
    uint32_t  slots0[1 + FM_OS_MAX_SLOTS];
};
struct DevRankSumArgs {
    DevOsCommon c;
    double*  partials;         // [batch][grid.x]
    double*  out_host;         // pinned [batch]
    uint32_t lo0, hi0;
};
struct DevCountArgs {
    DevOsCommon c;
    uint32_t* counts_dev;      // [m + 1]
    uint32_t* counts_host;     // pinned [m + 1]
    uint32_t  m, pow2;         // bounds; the largest power of two <= m
};
// workgroups per vector of a counting pass: a function of n and the batch size only
inline uint32_t os_blocks_per_vector(int64_t n, uint32_t batch)
{
    // Measured (profiles/order_statistics.json): a pass is bound by its counting and by what every workgroup does once —
    // clearing and flushing its histogram with global adds, being counted —, not by memory.  A workgroup per tile up to one workgroup per
    // CU (a 10^5-path vector: 145 -> 89 µs per quantile against four tiles each); beyond that four tiles (64 KB) per workgroup (10^7 paths:
    // 325 µs against 684 with a workgroup per tile), and about eight workgroups per CU for the whole batch at most.
    const int64_t tiles = (n + FM_OS_TILE - 1) / FM_OS_TILE;
    int64_t b = tiles <= 256 ? tiles : (tiles + 3) / 4;
    if (tiles > 256 && b < 256) b = 256;
    const int64_t cap = batch >= 2048u ? 1 : 2048 / (int64_t)(batch ? batch : 1u);
    if (b > cap) b = cap;
    return (uint32_t)(b < 1 ? 1 : b);
}
// workgroups per vector of the rank-sum pass: a function of n ONLY — the order of the fp64 additions depends on nothing else
inline uint32_t os_sum_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_OS_TILE - 1) / FM_OS_TILE;
    int64_t b = tiles;
    if (b > 1024) b = 1024;
    return (uint32_t)(b < 1 ? 1 : b);
}
// vecs: [batch] addresses; slots: [batch][1 + S] = {number of prefixes, prefixes …} (both unused with use_inline)
hipError_t launch_os_hist(const DevSelectArgs& a, const uint64_t* vecs, const uint32_t* slots, uint32_t batch, hipStream_t st);
// keys: [batch][2] = {key_lo, key_hi}, both exclusive
hipError_t launch_os_sum(const DevRankSumArgs& a, const uint64_t* vecs, const uint32_t* keys, uint32_t batch, hipStream_t st);
// bounds: [m] ascending doubles on the device; counts[i] = elements x (not NaN) with exactly i bounds < x
hipError_t launch_os_count(const DevCountArgs& a, const double* bounds, hipStream_t st);

// ---- cross moments (cross_moments_engine.hpp): S[i][j] = Σ_p x_i[p]·x_j[p] and T[i][m] = Σ_p x_i[p]·y_m[p] in fp64 for up
// to 12 + 4 vectors of one size, in ONE launch.  The vectors form one list (x then y; an address of 0 is the constant 1 and is not loaded);
// the list is cut into groups of FM_XMOM_GROUP = 8 and blockIdx.y names a pair of groups: a workgroup reads the (at most 16) vectors of its
// two groups once per tile and keeps all 8 x 8 products' running sums in registers.  Up to 8 vectors that is one block and every vector is
// read once; 9 … 16 vectors are three blocks (two when the second group holds dependents only) and 2 x the bytes at most.  The order of
// the additions of ONE pair — lane, tile by tile; butterfly over the lanes; waves; workgroups, lane-strided, by the last to arrive — depends
// on n alone: not on the block the pair falls into, the number of vectors, their roles or their positions.
constexpr int FM_XMOM_MAX_X = 12;
constexpr int FM_XMOM_MAX_Y = 4;
constexpr int FM_XMOM_GROUP = 8;
constexpr int FM_XMOM_PAIRS = FM_XMOM_GROUP * FM_XMOM_GROUP;      // running sums per workgroup
constexpr int FM_XMOM_MAX_BLOCKS = 3;                             // (0,0) (0,1) (1,1)
constexpr int FM_XMOM_TILE = 1024;                                // elements per workgroup and iteration: 256 lanes x 16 bytes
struct DevXmomArgs {
    uint32_t* counters;        // [FM_XMOM_MAX_BLOCKS + 1] arrival counters: one per block, one for the launch; zero before and after
    uint64_t* done_flag;       // pinned; receives done_value when out_host is in host memory
    uint64_t  done_value;
    int64_t   n;
    uint32_t  tiles;           // ceil(n / FM_XMOM_TILE)
    uint32_t  n_blocks;
    double*   partials;        // [n_blocks][FM_XMOM_PAIRS][grid.x]
    double*   out_host;        // pinned [n_blocks][FM_XMOM_PAIRS]: entry r * 8 + c = Σ (row group)[r] · (column group)[c]
    uint64_t  vec[2 * FM_XMOM_GROUP];            // addresses; 0 = the constant 1 (also what pads a group)
    uint8_t   row_group[4], col_group[4];        // per block
};
// workgroups per block: a function of n ONLY — the order of the fp64 additions depends on nothing else
inline uint32_t xmom_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_XMOM_TILE - 1) / FM_XMOM_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > 512 ? 512 : tiles);
}
hipError_t launch_xmom(const DevXmomArgs& a, hipStream_t st);

} // namespace fm
