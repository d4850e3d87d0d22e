// prefix_device.hpp — the device half of the tree of prefix_host.hpp: a lane's load of its 8 elements of a tile and the scan of a tile
// (levels 1 … 5), shared by every kernel that makes prefixes in that tree (prefix_kernel.hip, resample_kernel.hip) so that all of them make
// a prefix by the SAME operations.  Device code only; included by .hip files.
#pragma once
#include <hip/hip_runtime.h>

#include "prefix_host.hpp"

namespace fm {

typedef float pf_f32x4 __attribute__((ext_vector_type(4)));

struct PfLoad { pf_f32x4 q[2]; };

// the lane's 8 consecutive elements of `tile`: two 16-byte loads
__device__ __forceinline__ PfLoad pf_load(const pf_f32x4* __restrict__ v, const uint32_t tile, const uint32_t n)
{
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;      // < n + tile < 2^32
    PfLoad l;
    l.q[0] = v[e0 < n ? e0 / 4u : 0u];
    l.q[1] = v[e0 + 4u < n ? e0 / 4u + 1u : 0u];
    return l;
}

// The prefixes of the lane's elements INSIDE THE CHUNK (levels 1 … 5 of the tree).  carry: the last prefix of the tile before, inside the
// chunk (not read for the chunk's first tile); it leaves as this tile's.  wave_total: four doubles of LDS, written again two tiles later.
// Every thread of the workgroup calls (one barrier).
__device__ __forceinline__ void pf_tile(const PfLoad& l, const uint32_t tile, const uint32_t n, const bool first_tile, double& carry, double* wave_total, double (&p)[FM_PREFIX_ITEMS])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
    // level 1: along the lane
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
        const double x = e0 + (uint32_t)i < n ? (double)l.q[i >> 2][i & 3] : -0.0;
        p[i] = i == 0 ? x : p[i - 1] + x;
    }
    // level 2: the lanes of a group — the base of lane k is the last prefix of lane k - 1
    double base = 0.0;
    {
        const uint32_t k_own = lane & (uint32_t)(FM_PREFIX_GROUP - 1), first = lane & ~(uint32_t)(FM_PREFIX_GROUP - 1);
        const double last = p[FM_PREFIX_ITEMS - 1];
        double run = __shfl(last, (int)first, 64);
#pragma unroll
        for (uint32_t k = 1; k < (uint32_t)FM_PREFIX_GROUP; ++k) {
            if (k_own == k) base = run;
            run = run + __shfl(last, (int)(first + k), 64);
        }
        if (k_own > 0u) {
#pragma unroll
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[i] = base + p[i];
        }
        // level 3: the groups of a wave (run: the group's last prefix, in every lane of the group)
        const uint32_t g_own = lane / (uint32_t)FM_PREFIX_GROUP;
        const double group_last = run;
        run = __shfl(group_last, 0, 64);
#pragma unroll
        for (uint32_t g = 1; g < (uint32_t)FM_PREFIX_GROUPS; ++g) {
            if (g_own == g) base = run;
            run = run + __shfl(group_last, (int)(g * (uint32_t)FM_PREFIX_GROUP), 64);
        }
        if (g_own > 0u) {
#pragma unroll
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[i] = base + p[i];
        }
        // level 4: the waves of a tile (run: the wave's last prefix, in every lane)
        if (lane == 0u) wave_total[wave] = run;
    }
    __syncthreads();
    double run = wave_total[0];
#pragma unroll
    for (uint32_t w = 1; w < (uint32_t)FM_PREFIX_WAVES; ++w) {
        if (wave == w) base = run;
        run = run + wave_total[w];
    }
    if (wave > 0u) {
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[i] = base + p[i];
    }
    // level 5: the tiles of a chunk (run: the tile's last prefix, in every thread)
    if (first_tile) carry = run;
    else {
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[i] = carry + p[i];
        carry = carry + run;
    }
}

} // namespace fm
