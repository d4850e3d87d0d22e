// xmom_wide_device.hpp — the device code fm_xmom_wide_kernel (xmom_wide_kernel.hip) and fm_xmom_poly_kernel
// (xmom_poly_kernel.hip, §4.15) share: the tile map, the MFMA step, the additions of the waves and of the workgroups —
// the TREE of xmom_wide_kernel.h, once; the arrival of the workgroups is side_pass_device.hpp's.  What differs between the two kernels is how a round's operands are obtained, and that is a policy:
//
//   struct Policy {
//       struct Raw;                                                     what a round's loads leave in registers
//       void init(const uint64_t* slots, uint32_t lane, uint32_t sub);  the lane picks its slots (LDS copy of the list)
//       void load(uint32_t c, int r, Raw& k) const;                     issue the loads of round r of chunk c
//       void form(uint32_t c, int r, const Raw& k, XwRound<NG>& o) const;   the MFMA operands of that round: paths past n are +0.0
//   };
//
// Two Raw buffers: the loads of a round are issued before the round before it is formed and multiplied.  Only device code includes this.
#pragma once
#include <hip/hip_runtime.h>

#include "side_pass_device.hpp"
#include "xmom_wide_kernel.h"

namespace fm {

typedef float xw_f32x4 __attribute__((ext_vector_type(4)));
typedef double xw_f64x4 __attribute__((ext_vector_type(4)));
typedef xw_f32x4 __attribute__((address_space(1))) xw_gfloat4;

// tile (g, h), g <= h, in the layout of four groups (xmom_wide_entry)
__device__ __forceinline__ constexpr int xw_tile(int g, int h) { return g * (2 * FM_XMOMW_MAX_GROUPS - 1 - g) / 2 + h; }

template <int NG>
struct XwRound { xw_f32x4 v[NG]; };

// what lies past n is +0.0 in every operand of the round whose first path (of this lane) is p0
template <int NG>
__device__ __forceinline__ void xw_zero_tail(XwRound<NG>& k, const int64_t p0, const int64_t n)
{
    if (p0 + 4 > n) {                                               // only in the last chunk
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j >= n) {
#pragma unroll
                for (int g = 0; g < NG; ++g) k.v[g][j] = 0.0f;
            }
    }
}

// 4 steps x NT tiles: step s sums over the paths 16r + 4k + s, k = the lane's sub-index, of the round
template <int NG>
__device__ __forceinline__ void xw_multiply(const XwRound<NG>& k, xw_f64x4 (&acc)[NG * (NG + 1) / 2])
{
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
}

// The pass: chunks of 64 paths, 16 MFMAs per chunk and tile, the waves in order, the workgroups in order (xmom_wide_kernel.h).
template <int NG, class Policy>
__device__ __forceinline__ void xw_pass(const DevXmomWideArgs& A, Policy& P)
{
    constexpr int NT = NG * (NG + 1) / 2;
    __shared__ double wave_part[FM_XMOMW_WAVES][FM_XMOMW_TILE_ENTRIES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t sub = lane >> 4;                                 // the k of this lane's operand

    // the slots arrive in the kernel arguments; a lane picks its own through LDS (an argument indexed by the lane would be a private copy)
    __shared__ uint64_t slots[FM_XMOMW_MAX];
#pragma unroll
    for (int i = 0; i < NG * FM_XMOMW_GROUP; ++i) if (tid == 0u) slots[i] = A.vec[i];
    __syncthreads();
    P.init(slots, lane, sub);

    xw_f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = xw_f64x4{ 0.0, 0.0, 0.0, 0.0 };

    const uint32_t stride = gridDim.x * FM_XMOMW_WAVES;
    uint32_t c = blockIdx.x * FM_XMOMW_WAVES + wave;                // wave-uniform: the loop below is taken by whole waves
    typename Policy::Raw r0, r1;                                    // two buffers: the loads of a round are issued before the round before it is multiplied
    XwRound<NG> k;
    if (c < A.chunks) P.load(c, 0, r0);
#pragma unroll 1
    while (c < A.chunks) {
        const uint32_t c_next = c + stride;
        P.load(c, 1, r1); P.form(c, 0, r0, k); xw_multiply<NG>(k, acc);
        P.load(c, 2, r0); P.form(c, 1, r1, k); xw_multiply<NG>(k, acc);
        P.load(c, 3, r1); P.form(c, 2, r0, k); xw_multiply<NG>(k, acc);
        if (c_next < A.chunks) P.load(c_next, 0, r0);
        P.form(c, 3, r1, k); xw_multiply<NG>(k, acc);
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
    if (!pass_arrive_last(A.counter, gridDim.x)) return;

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

// The wide kernel's policy and the address slots of the polynomial kernel: a slot above FM_XMOMW_ONE is an address, loaded with four 16-byte
// loads per chunk; FM_XMOMW_ONE is the constant 1, FM_XMOMW_PAD a zero operand; neither is loaded.  TERMS: a slot tagged FM_XMOMW_TERM (a monomial the lane
// forms itself, xmom_poly_kernel.hip) is no address either and is left +0.0 here.
template <int NG, bool TERMS>
struct XwAddressLoads {
    uint64_t base[NG];                                              // 0: nothing to load
    float fill[NG];
    __device__ __forceinline__ void init(const uint64_t* slots, const uint32_t lane, const uint32_t sub)
    {
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint64_t slot = slots[g * FM_XMOMW_GROUP + (lane & 15u)];
            base[g] = (slot > FM_XMOMW_ONE && !(TERMS && (slot & FM_XMOMW_TERM))) ? slot + sub * 16u : 0ull;
            fill[g] = slot == FM_XMOMW_ONE ? 1.0f : 0.0f;
        }
    }
    // round r of chunk c: the paths c·64 + 16r + 4·sub … + 3 of this lane's vector of every group
    __device__ __forceinline__ void load(const uint32_t c, const int r, XwRound<NG>& k) const
    {
        const uint64_t at = (uint64_t)c * (FM_XMOMW_CHUNK * 4) + (uint64_t)r * 64u;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            xw_f32x4 v = { fill[g], fill[g], fill[g], fill[g] };
            if (base[g]) v = *reinterpret_cast<const xw_gfloat4*>(base[g] + at);
            k.v[g] = v;
        }
    }
};

} // namespace fm
