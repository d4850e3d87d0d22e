// sobol_kernel.hip — fm_sobol_bm_kernel: Brownian increments from Sobol' points on gfx950 (MI355X, CDNA4).  DESIGN.md §4.12; the definition
// is host/sobol.hpp, whose point, uniform, normal quantile and bridge node this file compiles from the same text as the host, so every
// increment EQUALS the host's narrowed to fp32.
//
// Shape.  One lane per path.  A workgroup owns 256 consecutive sequence indices i (i = global path + 1) ALIGNED to 256, so
//   * every store of a (step, factor) vector is a run of 64 consecutive floats per wave (nontemporal: nothing here reads them again);
//   * the Gray code i ^ (i >> 1) splits into bits 8 … 29, which depend on the workgroup alone, and bits 0 … 7, which depend on the lane:
//     x(i, d) is one XOR chain over the SET high bits per dimension (wave-uniform: scalar loads and scalar XORs, about log2(index) / 2 of
//     them, started from the dimension's digital shift) and eight select-and-XOR per lane.  No draw walks 30 bits.
// Direction words.  The engine uploads the 30 words of every dimension in use (at most 120 KB) once per call; the kernel reads
// them with wave-uniform addresses, through the scalar cache.  Per dimension a workgroup reads 8 + popcount(high bits) + 1 words (some 60 B
// at 10^6 paths) and stores 1 KB: below 6 % of its store traffic, all of it hits in L2 after the first workgroups.  Staging through LDS
// would take the LDS the bridge wants, and a pre-folding launch would write and read 4 B per (workgroup, dimension) to save these reads: neither pays.
// Bridge.  The lanes walk the host's plan (fmhost::SobolOp, 32 B per step, wave-uniform) once per factor: nodes in TIME order, each W in one
// of n_slots <= 16 slots (12 at 1024 steps), a column of doubles per lane in LDS (slot · 256 + lane: a lane reads only what it wrote, so
// there is no barrier, and consecutive lanes hit consecutive 8-byte words: no bank conflict).  LDS: n_slots · 2 KB, dynamic — 20 KB at 200
// steps, none for the incremental construction.  No array is indexed in registers: 0 bytes of scratch (tests/test_sobol_cpu.py).
// The kernel trusts its arguments: launch_sobol_bm refuses what sobol_shape_ok refuses, and the engine validates the plan (sobolPlanOk).
#include <hip/hip_runtime.h>

#include "sobol_kernel.h"

namespace fm {

struct SobolShape {
    int64_t  stride_floats, n_paths, path_offset;
    uint32_t n_ops, n_factors, n_slots, first_block;
};

__global__ void __launch_bounds__(FM_SOBOL_BLOCK) fm_sobol_bm_kernel(float* __restrict__ slab, const uint32_t* __restrict__ directions,
                                                                     const uint32_t* __restrict__ shifts, const fmhost::SobolOp* __restrict__ ops,
                                                                     const SobolShape S)
{
    extern __shared__ double W[];                                           // [n_slots][FM_SOBOL_BLOCK]
    const uint32_t lane = threadIdx.x;
    const uint32_t base = (S.first_block + blockIdx.x) << FM_SOBOL_BLOCK_LOG2;
    const uint32_t i = base + lane;
    const int64_t local = (int64_t)i - 1 - S.path_offset;                   // the first and the last workgroup may reach beyond the block of paths
    const bool live = local >= 0 && local < S.n_paths;
    const uint32_t gray = i ^ (i >> 1);
    const uint32_t gray_high = (base ^ (base >> 1)) >> FM_SOBOL_BLOCK_LOG2; // bits 8 … 29 of every lane's Gray code
    if (S.n_slots) W[lane] = 0.0;                                           // slot 0: W(t_0)

    for (uint32_t f = 0; f < S.n_factors; ++f) {
        for (uint32_t k = 0; k < S.n_ops; ++k) {
            const fmhost::SobolOp o = ops[k];
            double z = 0.0;
            if (o.kind != fmhost::FM_SOBOL_OP_EMIT) {
                const uint32_t d = o.node * S.n_factors + f;
                const uint32_t* __restrict__ v = directions + (size_t)d * fmhost::FM_SOBOL_BITS;
                uint32_t x = shifts[d];
                for (uint32_t h = gray_high; h; h &= h - 1) x ^= v[FM_SOBOL_BLOCK_LOG2 + __builtin_ctz(h)];
#pragma unroll
                for (int j = 0; j < FM_SOBOL_BLOCK_LOG2; ++j) x ^= ((gray >> j) & 1u) ? v[j] : 0u;
                z = fmhost::fm_normal_quantile(fmhost::fm_sobol_uniform(x));
            }
            double increment;
            if (o.kind == fmhost::FM_SOBOL_OP_DRAW) increment = z * o.sd;
            else if (o.kind == fmhost::FM_SOBOL_OP_EMIT) increment = W[(uint32_t)o.right * FM_SOBOL_BLOCK + lane] - W[(uint32_t)o.left * FM_SOBOL_BLOCK + lane];
            else {
                W[(uint32_t)o.out * FM_SOBOL_BLOCK + lane] = o.kind == fmhost::FM_SOBOL_OP_TERMINAL
                    ? o.sd * z
                    : fmhost::fm_bridge_node(o.a, o.b, o.sd, W[(uint32_t)o.left * FM_SOBOL_BLOCK + lane], W[(uint32_t)o.right * FM_SOBOL_BLOCK + lane], z);
                continue;
            }
            if (live) __builtin_nontemporal_store((float)increment, slab + ((size_t)o.node * S.n_factors + f) * (size_t)S.stride_floats + (size_t)local);
        }
    }
}

hipError_t launch_sobol_bm(const DevSobolArgs& a, hipStream_t st)
{
    if (a.n_paths <= 0) return hipSuccess;
    if (!sobol_shape_ok(a)) return hipErrorInvalidValue;
    const SobolShape S{ a.stride_floats, a.n_paths, a.path_offset, a.n_ops, a.n_factors, a.n_slots, a.first_block };
    hipLaunchKernelGGL(fm_sobol_bm_kernel, dim3(a.n_blocks), dim3(FM_SOBOL_BLOCK), (size_t)a.n_slots * FM_SOBOL_BLOCK * sizeof(double), st,
                       a.slab, a.directions, a.shifts, a.ops, S);
    return hipGetLastError();
}

} // namespace fm
