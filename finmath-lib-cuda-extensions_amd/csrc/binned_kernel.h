// binned_kernel.h — host-callable launchers of the two kernels of binned_kernel.hip (engine side: binned_engine.hpp;
// definition: host/binned_regression.hpp): the cross moments of up to 3 + 4 vectors PER BIN of a key vector in one pass, and the
// piecewise-linear estimate evaluated as a new vector.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fm {

constexpr int FM_BINNED_MAX_BINS = 64;
constexpr int FM_BINNED_MAX_X = 3;
constexpr int FM_BINNED_MAX_Y = 4;
constexpr int FM_BINNED_SLOTS = FM_BINNED_MAX_X * (FM_BINNED_MAX_X + 1) / 2 + FM_BINNED_MAX_X * FM_BINNED_MAX_Y;      // 18 products at most
constexpr int FM_BINNED_BLOCK = 256;
constexpr int FM_BINNED_TILE = 1024;               // elements per workgroup and iteration: 256 lanes x 16 bytes
// Lane-private running sums in LDS, [entry][lane]: FM_BINNED_ENTRIES x 256 x 8 B = 144 KB of the CU's 160 KB (one workgroup per CU).  An
// entry is one (bin, product); a launch whose bins x products exceed the entries cuts the BINS into slices along blockIdx.y.
constexpr int FM_BINNED_ENTRIES = 72;
constexpr int FM_BINNED_MAX_SLICES = FM_BINNED_MAX_BINS;

// The 18 slots are the products of the FULL shape (3 x, 4 y) in the layout of fmhip_cross_moments: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), then
// x_i·y_m at 6 + 4·i + m.  slot_entry[s] is the slot's entry inside a bin (0 … entries_per_bin - 1), or -1 for a product the call does not ask
// for — and for (1, 1) of two constants, which is the bin's count.
struct DevBinnedXmomArgs {
    uint32_t* counters;        // [FM_BINNED_MAX_SLICES + 1] arrival counters: one per slice, one for the launch; zero before and after
    uint32_t* counts_dev;      // [FM_BINNED_MAX_BINS] zero before and after
    uint64_t* done_flag;       // pinned; receives done_value when counts_host and out_host are in host memory
    uint64_t  done_value;
    int64_t   n;
    uint32_t  tiles;           // ceil(n / FM_BINNED_TILE)
    uint32_t  n_bins;
    uint32_t  entries_per_bin; // 1 … 18
    uint32_t  bins_per_slice;  // entries_per_bin * bins_per_slice <= FM_BINNED_ENTRIES
    uint32_t  n_slices;        // ceil(n_bins / bins_per_slice) = gridDim.y
    uint32_t  n_x, n_y;
    const double* bounds;      // device, [n_bins - 1] ascending
    double*   partials;        // [n_slices][FM_BINNED_ENTRIES][grid.x]
    double*   out_host;        // pinned [n_bins][entries_per_bin]
    uint32_t* counts_host;     // pinned [n_bins]
    uint64_t  key;             // address of the key vector
    uint64_t  x[FM_BINNED_MAX_X], y[FM_BINNED_MAX_Y];      // addresses; an x of 0 = the constant 1
    int8_t    slot_entry[FM_BINNED_SLOTS + 2];
};
// workgroups along x: a function of n ONLY — the order of the fp64 additions of one (bin, product) depends on nothing else
inline uint32_t binned_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_BINNED_TILE - 1) / FM_BINNED_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > 256 ? 256 : tiles);
}
inline bool binned_xmom_shape_ok(const DevBinnedXmomArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31) || a.tiles != (uint32_t)((a.n + FM_BINNED_TILE - 1) / FM_BINNED_TILE)) return false;
    if (a.n_bins < 1 || a.n_bins > (uint32_t)FM_BINNED_MAX_BINS || a.n_x < 1 || a.n_x > (uint32_t)FM_BINNED_MAX_X || a.n_y > (uint32_t)FM_BINNED_MAX_Y) return false;
    if (a.entries_per_bin < 1 || a.entries_per_bin > (uint32_t)FM_BINNED_SLOTS || a.bins_per_slice < 1) return false;
    if (a.entries_per_bin * a.bins_per_slice > (uint32_t)FM_BINNED_ENTRIES) return false;
    if (a.n_slices != (a.n_bins + a.bins_per_slice - 1) / a.bins_per_slice || a.n_slices > (uint32_t)FM_BINNED_MAX_SLICES) return false;
    if (!a.key || (a.n_bins > 1 && !a.bounds) || !a.counters || !a.counts_dev || !a.partials || !a.out_host || !a.counts_host || !a.done_flag) return false;
    for (uint32_t m = 0; m < a.n_y; ++m) if (!a.y[m]) return false;
    for (int s = 0; s < FM_BINNED_SLOTS; ++s) if (a.slot_entry[s] < -1 || a.slot_entry[s] >= (int)a.entries_per_bin) return false;
    return true;
}
hipError_t launch_binned_xmom(const DevBinnedXmomArgs& a, hipStream_t st);

struct DevBinnedEvalArgs {
    int64_t   n;
    uint32_t  n_bins, n_x;
    const double* bounds;      // device, [n_bins - 1]
    const float*  coefficients;// device, [n_bins][n_x], narrowed on the host
    uint64_t  key, out;        // addresses (vectors are padded to 256 B)
    uint64_t  x[FM_BINNED_MAX_X];
};
inline bool binned_eval_shape_ok(const DevBinnedEvalArgs& a)
{
    return a.n > 0 && a.n <= (int64_t(1) << 31) && a.n_bins >= 1 && a.n_bins <= (uint32_t)FM_BINNED_MAX_BINS && a.n_x >= 1 && a.n_x <= (uint32_t)FM_BINNED_MAX_X
        && a.key && a.out && a.coefficients && (a.n_bins == 1 || a.bounds);
}
hipError_t launch_binned_eval(const DevBinnedEvalArgs& a, hipStream_t st);

} // namespace fm
