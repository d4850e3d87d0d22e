// xmom_wide_kernel.hip — fm_xmom_wide_kernel for gfx950 (MI355X, CDNA4): the normal equations of a least-squares regression on up to 64
// vectors — XᵀX — in one pass, on the matrix cores.  DESIGN.md §4.14; contract: include/fmhip.h; layout, tree and L(n): xmom_wide_kernel.h;
// engine side: xmom_wide_engine.hpp.
//
// v_mfma_f64_16x16x4_f64 computes D = A·B + C for a 16 x 4 A, a 4 x 16 B and a 16 x 16 C/D.  Lane l holds ONE f64 of A, A[l & 15][l >> 4], and
// one of B, B[l >> 4][l & 15]; C/D are 4 f64 per lane, col = l & 15, row = (l >> 4) + 4·reg (this is NOT the f32 forms' row formula).
// With rows of A = vectors of group g, columns of B = vectors of group h and k = a path, lane l needs x_{16g + (l & 15)} at path p + (l >> 4)
// as the A operand of group g AND as the B operand of group g: one register serves both, no transpose, no LDS staging, no second load.
//
// Loads.  A wave takes a chunk of 64 paths: per group four 16-byte loads per lane, load r from vector (l & 15) at path 16r + 4·(l >> 4).  The
// four floats of a load feed four MFMA steps; step s sums over the paths 16r + 4k + s, k = 0 … 3 — both operands use the same path-to-k
// map, which is all that correctness asks.  The wave reads whole 256-byte lines of every vector, and a round's loads are issued before
// the MFMAs of the round before it.  A vector's storage is padded to 256 bytes, so every chunk that starts below n is in bounds; paths past
// n are +0.0 in both operands, the constant 1 included.
//
// A product of two fp32 values is exact in fp64, so every step adds exact products; what rounds is the running sum.  No fp32 product, no
// float atomics.  The tree is in xmom_wide_kernel.h.  The kernel trusts its arguments: the launcher refuses what xmom_wide_shape_ok
// refuses.  No register array is indexed at run time: no scratch.
#include <hip/hip_runtime.h>

#include "xmom_wide_kernel.h"

namespace fm {

typedef float xw_f32x4 __attribute__((ext_vector_type(4)));
typedef double xw_f64x4 __attribute__((ext_vector_type(4)));
typedef xw_f32x4 __attribute__((address_space(1))) xw_gfloat4;

// true, for the whole workgroup, in the LAST of `members` workgroups to arrive at `counter` (zero before the launch, zero again after the
// last arrival); what the others wrote before they arrived is visible to it (fm_xmom_kernel's protocol: release, agent-scope add, acquire)
__device__ __forceinline__ bool xw_arrive_last(uint32_t* counter, const uint32_t members, uint32_t* last)
{
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t arrived = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        *last = (arrived == members - 1u) ? 1u : 0u;
        if (*last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const bool r = *last != 0u;
    if (r) __threadfence();
    return r;
}

// tile (g, h), g <= h, in the layout of four groups (xmom_wide_entry)
__device__ __forceinline__ constexpr int xw_tile(int g, int h) { return g * (2 * FM_XMOMW_MAX_GROUPS - 1 - g) / 2 + h; }

template <int NG>
struct XwRound { xw_f32x4 v[NG]; };

template <int NG>
__global__ void __launch_bounds__(FM_XMOMW_BLOCK) fm_xmom_wide_kernel(const DevXmomWideArgs A)
{
    constexpr int NT = NG * (NG + 1) / 2;
    __shared__ double wave_part[FM_XMOMW_WAVES][FM_XMOMW_TILE_ENTRIES];
    __shared__ uint32_t last;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t sub = lane >> 4;                                 // the k of this lane's operand
    const int64_t n = A.n;

    // the slots arrive in the kernel arguments; a lane picks its own through LDS (an argument indexed by the lane would be a private copy)
    __shared__ uint64_t slots[FM_XMOMW_MAX];
#pragma unroll
    for (int i = 0; i < NG * FM_XMOMW_GROUP; ++i) if (tid == 0u) slots[i] = A.vec[i];
    __syncthreads();
    uint64_t base[NG];                                              // 0: nothing to load
    float fill[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const uint64_t slot = slots[g * FM_XMOMW_GROUP + (lane & 15u)];
        base[g] = slot > FM_XMOMW_ONE ? slot + sub * 16u : 0ull;
        fill[g] = slot == FM_XMOMW_ONE ? 1.0f : 0.0f;
    }

    // round r of chunk c: the paths c·64 + 16r + 4·sub … + 3 of this lane's vector of every group
    auto load = [&](const uint32_t c, const int r, XwRound<NG>& k) {
        const uint64_t at = (uint64_t)c * (FM_XMOMW_CHUNK * 4) + (uint64_t)r * 64u;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            xw_f32x4 v = { fill[g], fill[g], fill[g], fill[g] };
            if (base[g]) v = *reinterpret_cast<const xw_gfloat4*>(base[g] + at);
            k.v[g] = v;
        }
        const int64_t p0 = (int64_t)c * FM_XMOMW_CHUNK + r * 16 + sub * 4u;
        if (p0 + 4 > n) {                                           // only in the last chunk: what lies past n is +0.0
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p0 + j >= n) {
#pragma unroll
                    for (int g = 0; g < NG; ++g) k.v[g][j] = 0.0f;
                }
        }
    };
    auto multiply = [&](const XwRound<NG>& k, xw_f64x4 (&acc)[NT]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            double op[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) op[g] = (double)k.v[g][s];
            int t = 0;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int h = g; h < NG; ++h, ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[g], op[h], acc[t], 0, 0, 0);
        }
    };

    xw_f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = xw_f64x4{ 0.0, 0.0, 0.0, 0.0 };

    const uint32_t stride = gridDim.x * FM_XMOMW_WAVES;
    uint32_t c = blockIdx.x * FM_XMOMW_WAVES + wave;                // wave-uniform: the loop below is taken by whole waves
    XwRound<NG> r0, r1;                                             // two buffers: the loads of a round are issued before the round before it is multiplied
    if (c < A.chunks) load(c, 0, r0);
#pragma unroll 1
    while (c < A.chunks) {
        const uint32_t c_next = c + stride;
        load(c, 1, r1); multiply(r0, acc);
        load(c, 2, r0); multiply(r1, acc);
        load(c, 3, r1); multiply(r0, acc);
        if (c_next < A.chunks) load(c_next, 0, r0);
        multiply(r1, acc);
        c = c_next;
    }

    // the waves of the workgroup, in order, tile by tile
    double* part = A.partials + (size_t)blockIdx.x * (FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES);
    {
        int t = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int h = g; h < NG; ++h, ++t) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) wave_part[wave][reg * 64 + lane] = acc[t][reg];
                __syncthreads();
                if (tid < (uint32_t)FM_XMOMW_TILE_ENTRIES) {
                    double s = wave_part[0][tid];
#pragma unroll
                    for (int w = 1; w < FM_XMOMW_WAVES; ++w) s += wave_part[w][tid];
                    part[xw_tile(g, h) * FM_XMOMW_TILE_ENTRIES + tid] = s;
                }
                __syncthreads();
            }
    }
    if (!xw_arrive_last(A.counter, gridDim.x, &last)) return;

    // the workgroups, in order: the two halves of the last workgroup take the tiles alternately, a thread one entry of each of its tiles
    {
        const uint32_t half = tid >> 8, e = tid & 255u;
        const double* from = A.partials + e;
        double s[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) s[t] = 0.0;
#pragma unroll 4
        for (uint32_t b = 0; b < gridDim.x; ++b) {
            const double* pb = from + (size_t)b * (FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES);
            int t = 0;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int h = g; h < NG; ++h, ++t)
                    if ((uint32_t)(t & 1) == half) { const double v = pb[xw_tile(g, h) * FM_XMOMW_TILE_ENTRIES]; s[t] = b == 0u ? v : s[t] + v; }
        }
        int t = 0;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int h = g; h < NG; ++h, ++t)
                if ((uint32_t)(t & 1) == half) A.out_host[xw_tile(g, h) * FM_XMOMW_TILE_ENTRIES + e] = s[t];
    }
    __threadfence_system();
    __syncthreads();
    if (tid == 0u) __hip_atomic_store(A.done_flag, A.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_xmom_wide(const DevXmomWideArgs& a, hipStream_t st)
{
    if (!xmom_wide_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(xmom_wide_blocks(a.n), 1, 1), block(FM_XMOMW_BLOCK);
    switch (a.n_groups) {
    case 1:  hipLaunchKernelGGL(fm_xmom_wide_kernel<1>, grid, block, 0, st, a); break;
    case 2:  hipLaunchKernelGGL(fm_xmom_wide_kernel<2>, grid, block, 0, st, a); break;
    case 3:  hipLaunchKernelGGL(fm_xmom_wide_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(fm_xmom_wide_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

} // namespace fm
