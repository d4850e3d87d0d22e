// null_sobol.cpp — TEST-ONLY stand-in for the launcher of fm_sobol_bm_kernel (sobol_kernel.hip).  It generates the plain way, one path after
// the other with the host code, from what the engine hands it — the PLAN, the DIRECTION WORDS and the SHIFTS of the upload, walked exactly
// as the kernel walks them (slots and all) — and rebuilds nothing from the caller's arguments: a wrong offset into the upload, a plan whose
// slots collide, a missing dimension or an undersized block is a wrong number or an ASan report in the driver (drive_sobol.cpp).
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdint>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/sobol_kernel.h"

namespace fm {

std::atomic<int> g_null_sobol_launches{ 0 }, g_null_sobol_slots{ 0 }, g_null_sobol_blocks{ 0 };     // launches so far; slots and workgroups of the last one

hipError_t launch_sobol_bm(const DevSobolArgs& a, hipStream_t) {
    if (a.n_paths <= 0) return hipSuccess;
    if (!sobol_shape_ok(a)) return hipErrorInvalidValue;
    if (!fmhost::sobolPlanOk(a.ops, a.n_ops, (int)a.n_steps, (int)a.n_factors, (int)a.n_slots)) return hipErrorInvalidValue;
    g_null_sobol_slots = (int)a.n_slots; g_null_sobol_blocks = (int)a.n_blocks; ++g_null_sobol_launches;
    std::vector<double> W((size_t)a.n_slots + 1, 0.0);
    // as the kernel: workgroups of 256 aligned indices, lanes outside the block of paths masked
    for (uint32_t block = 0; block < a.n_blocks; ++block)
        for (uint32_t lane = 0; lane < (uint32_t)FM_SOBOL_BLOCK; ++lane) {
            const uint32_t i = ((a.first_block + block) << FM_SOBOL_BLOCK_LOG2) + lane;
            const int64_t local = (int64_t)i - 1 - a.path_offset;
            if (local < 0 || local >= a.n_paths) continue;
            for (uint32_t f = 0; f < a.n_factors; ++f) {
                W[0] = 0.0;
                for (uint32_t k = 0; k < a.n_ops; ++k) {
                    const fmhost::SobolOp& o = a.ops[k];
                    double z = 0.0;
                    if (o.kind != fmhost::FM_SOBOL_OP_EMIT) {
                        const uint32_t d = o.node * a.n_factors + f;
                        z = fmhost::fm_normal_quantile(fmhost::fm_sobol_uniform(fmhost::fm_sobol_point(a.directions + (size_t)d * fmhost::FM_SOBOL_BITS, i) ^ a.shifts[d]));
                    }
                    double increment;
                    if (o.kind == fmhost::FM_SOBOL_OP_DRAW) increment = z * o.sd;
                    else if (o.kind == fmhost::FM_SOBOL_OP_EMIT) increment = W[o.right] - W[o.left];
                    else { W[o.out] = o.kind == fmhost::FM_SOBOL_OP_TERMINAL ? o.sd * z : fmhost::fm_bridge_node(o.a, o.b, o.sd, W[o.left], W[o.right], z); continue; }
                    a.slab[((size_t)o.node * a.n_factors + f) * (size_t)a.stride_floats + (size_t)local] = (float)increment;
                }
            }
        }
    return hipSuccess;
}

} // namespace fm
