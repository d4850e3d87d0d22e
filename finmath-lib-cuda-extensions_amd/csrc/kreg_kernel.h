// kreg_kernel.h — host-callable launcher of fm_kernel_moments_kernel (kreg_kernel.hip; engine side: kreg_engine.hpp;
// definition: host/kernel_regression.hpp): the kernel-weighted local moments of up to 4 vectors at up to 256 points of a key vector in one
// pass.  The accumulator layout, the reduction tree and the grid along x are those of the binned pass (binned_kernel.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "binned_kernel.h"

namespace fm {

constexpr int FM_KREG_MAX_POINTS = 256;
constexpr int FM_KREG_MAX_Y = 4;
constexpr int FM_KREG_BLOCK = FM_BINNED_BLOCK;         // 256 lanes
constexpr int FM_KREG_TILE = FM_BINNED_TILE;           // 1024 elements per workgroup and iteration: 256 lanes x 16 bytes
// Lane-private running sums in LDS, [entry][lane]: 72 x 256 x 8 B = 144 KB (one workgroup per CU).  An entry is one (point, term); a launch
// whose points x terms exceed the entries cuts the POINTS into slices along blockIdx.y.
constexpr int FM_KREG_ENTRIES = FM_BINNED_ENTRIES;
constexpr int FM_KREG_MAX_ENTRIES_PER_POINT = 3 + 2 * FM_KREG_MAX_Y;       // 11: 256 points are 43 slices of 6 points then
constexpr int FM_KREG_MAX_SLICES = 64;
constexpr int FM_KREG_PAD = 512;                       // lower and upper in LDS, padded with +inf to the power of two above the number of points

struct DevKernelMomentsArgs {
    uint32_t* counters;        // [FM_KREG_MAX_SLICES + 1] arrival counters: one per slice, one for the launch; zero before and after
    uint64_t* done_flag;       // pinned; receives done_value when out_host is in host memory
    uint64_t  done_value;
    int64_t   n;
    uint32_t  tiles;           // ceil(n / FM_KREG_TILE)
    uint32_t  n_points;        // Q: 1 … 256
    uint32_t  search_half;     // half the power of two above Q: 1 … 256 — the first step of the two lower-bound searches
    uint32_t  kernel;          // fmhost::FM_KERNEL_*
    uint32_t  order;           // 0 or 1
    uint32_t  n_y;             // 0 … 4
    uint32_t  entries_per_point;   // order 0: 1 + n_y, order 1: 3 + 2 n_y
    uint32_t  points_per_slice;    // entries_per_point * points_per_slice <= FM_KREG_ENTRIES
    uint32_t  n_slices;        // ceil(n_points / points_per_slice) = gridDim.y
    const double* tables;      // device: lower[Q] upper[Q] points[Q] rh[Q]
    double*   partials;        // [n_slices][FM_KREG_ENTRIES][grid.x]
    double*   out_host;        // pinned [n_points][entries_per_point]
    uint64_t  key;             // address of the key vector
    uint64_t  y[FM_KREG_MAX_Y];
};
// workgroups along x: binned_blocks(n), a function of n ONLY — the order of the fp64 additions of one (point, term) depends on nothing else
inline bool kernel_moments_shape_ok(const DevKernelMomentsArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31) || a.tiles != (uint32_t)((a.n + FM_KREG_TILE - 1) / FM_KREG_TILE)) return false;
    if (a.n_points < 1 || a.n_points > (uint32_t)FM_KREG_MAX_POINTS || a.n_y > (uint32_t)FM_KREG_MAX_Y || a.order > 1u || a.kernel > 4u) return false;
    if (a.search_half < 1 || (a.search_half & (a.search_half - 1)) != 0 || 2 * a.search_half <= a.n_points || a.search_half > a.n_points || 2 * a.search_half > (uint32_t)FM_KREG_PAD) return false;
    if (a.entries_per_point != (a.order == 0 ? 1 + a.n_y : 3 + 2 * a.n_y) || a.points_per_slice < 1) return false;
    if (a.entries_per_point * a.points_per_slice > (uint32_t)FM_KREG_ENTRIES) return false;
    if (a.n_slices != (a.n_points + a.points_per_slice - 1) / a.points_per_slice || a.n_slices > (uint32_t)FM_KREG_MAX_SLICES) return false;
    if (!a.key || !a.tables || !a.counters || !a.partials || !a.out_host || !a.done_flag) return false;
    for (uint32_t m = 0; m < a.n_y; ++m) if (!a.y[m]) return false;
    return true;
}
hipError_t launch_kernel_moments(const DevKernelMomentsArgs& a, hipStream_t st);

} // namespace fm
