// sobol_kernel.h — host-callable launcher of fm_sobol_bm_kernel (sobol_kernel.hip): Brownian increments from Sobol' points, with a Brownian
// bridge or increment by increment (definition: host/sobol.hpp).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/sobol.hpp"

namespace fm {

constexpr int FM_SOBOL_BLOCK = 256;                // threads of a workgroup = consecutive sequence indices it owns, aligned to its size
constexpr int FM_SOBOL_BLOCK_LOG2 = 8;

struct DevSobolArgs {
    float*                  slab;           // n_steps · n_factors vectors, `stride_floats` apart
    int64_t                 stride_floats;
    const uint32_t*         directions;     // [n_dims][30] expanded direction words, n_dims = n_steps · n_factors
    const uint32_t*         shifts;         // [n_dims] digital shift (all 0 without randomisation)
    const fmhost::SobolOp*  ops;            // [n_ops] the plan, walked once per factor
    int64_t                 n_paths;        // paths held by this process
    int64_t                 path_offset;    // global index of local path 0; the point of global path p is i = p + 1
    uint32_t                n_ops, n_steps, n_factors, n_slots;
    uint32_t                first_block;    // (path_offset + 1) / FM_SOBOL_BLOCK: workgroup b owns indices (first_block + b) · 256 … + 255
    uint32_t                n_blocks;       // workgroups
};

// What the kernel relies on in its arguments and does not check itself; the launcher refuses anything else, and so does the stand-in of
// the null device (tests/nulldev/null_sobol.cpp), which can look into the plan as well.
inline bool sobol_shape_ok(const DevSobolArgs& a)
{
    if (!a.slab || !a.directions || !a.shifts || !a.ops || ((uintptr_t)a.ops & 7u) || ((uintptr_t)a.directions & 3u) || ((uintptr_t)a.shifts & 3u)) return false;
    if (a.n_paths <= 0 || a.path_offset < 0 || a.stride_floats < a.n_paths) return false;
    if (a.n_steps == 0 || a.n_factors == 0 || (uint64_t)a.n_steps * a.n_factors > (uint64_t)fmhost::FM_SOBOL_DIMS) return false;
    if (a.n_ops == 0 || a.n_ops > 2 * a.n_steps || a.n_slots > (uint32_t)fmhost::FM_SOBOL_MAX_SLOTS) return false;
    const int64_t first = a.path_offset + 1, last = a.path_offset + a.n_paths;                    // indices drawn
    if (last >= fmhost::FM_SOBOL_INDEX_LIMIT) return false;
    return a.first_block == (uint32_t)(first >> FM_SOBOL_BLOCK_LOG2) && a.n_blocks == (uint32_t)((last >> FM_SOBOL_BLOCK_LOG2) - (first >> FM_SOBOL_BLOCK_LOG2) + 1);
}

hipError_t launch_sobol_bm(const DevSobolArgs& a, hipStream_t st);

} // namespace fm
