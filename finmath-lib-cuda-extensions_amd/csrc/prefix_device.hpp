// prefix_device.hpp — the device half of the tree of prefix_host.hpp: a lane's load of its 8 elements of a tile and the scan of a tile
// (levels 1 … 5), shared by every kernel that makes prefixes in that tree (prefix_kernel.hip, resample_kernel.hip, and with head flags
// group_kernel.hip) so that all of them make a prefix by the SAME operations.  Device code only; included by .hip files.
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

// What a segmented scan (group_kernel.hip; the rule of group_host.hpp) adds to a tile: in, `heads` — bit i is set where the lane's element
// i starts a run; out, `open` — bit i is set where no head lies at or before element i inside the TILE — and `any`: the tile holds a head.
struct PfSeg { uint32_t heads, open; bool any; };

// The prefixes of the lane's elements INSIDE THE CHUNK (levels 1 … 5 of the tree); p enters as the lane's terms (-0.0 past n).  carry: the
// last prefix of the tile before, inside the chunk (not read for the chunk's first tile); it leaves as this tile's.  wave_total: four doubles
// of LDS, written again two tiles later.  Every thread of the workgroup calls (one barrier).
// SEG: run-prefixes — a base is added only to the elements of the run that is open at the subunit's start, and a subunit that holds a head
// hands on its own last run-prefix, not the sum with what came before.  wave_head: four words of LDS beside wave_total.  Without SEG, seg
// and wave_head are not looked at and the operations are the plain tree's.
template <bool SEG>
__device__ __forceinline__ void pf_tile_terms(const bool first_tile, double& carry, double* wave_total, double (&p)[FM_PREFIX_ITEMS], PfSeg& seg, uint32_t* wave_head)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // level 1: along the lane
#pragma unroll
    for (int i = 1; i < FM_PREFIX_ITEMS; ++i) {
        if (SEG) { if (!((seg.heads >> i) & 1u)) p[i] = p[i - 1] + p[i]; }
        else p[i] = p[i - 1] + p[i];
    }
    // the lane's elements before its first head, and the lanes of the wave that hold one
    const uint32_t open_lane = !SEG ? 0xffu : seg.heads == 0u ? 0xffu : (1u << (uint32_t)__builtin_ctz(seg.heads)) - 1u;
    const uint64_t lanes = SEG ? (uint64_t)__ballot(seg.heads != 0u) : 0ull;
    uint32_t open = open_lane;
    // level 2: the lanes of a group — the base of lane k is the last prefix of lane k - 1
    double base = 0.0;
    {
        const uint32_t k_own = lane & (uint32_t)(FM_PREFIX_GROUP - 1), first = lane & ~(uint32_t)(FM_PREFIX_GROUP - 1);
        const double last = p[FM_PREFIX_ITEMS - 1];
        double run = __shfl(last, (int)first, 64);
#pragma unroll
        for (uint32_t k = 1; k < (uint32_t)FM_PREFIX_GROUP; ++k) {
            if (k_own == k) base = run;
            const double next = __shfl(last, (int)(first + k), 64);
            if (SEG) run = ((lanes >> (first + k)) & 1ull) ? next : run + next;
            else run = run + next;
        }
        if (k_own > 0u) {
#pragma unroll
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (!SEG || ((open >> i) & 1u)) p[i] = base + p[i];
        }
        if (SEG && ((lanes >> first) & ((1ull << k_own) - 1ull)) != 0ull) open = 0u;          // a head in an earlier lane of the group
        // level 3: the groups of a wave (run: the group's last prefix, in every lane of the group)
        const uint32_t g_own = lane / (uint32_t)FM_PREFIX_GROUP;
        const double group_last = run;
        run = __shfl(group_last, 0, 64);
#pragma unroll
        for (uint32_t g = 1; g < (uint32_t)FM_PREFIX_GROUPS; ++g) {
            if (g_own == g) base = run;
            const double next = __shfl(group_last, (int)(g * (uint32_t)FM_PREFIX_GROUP), 64);
            if (SEG) run = ((lanes >> (g * (uint32_t)FM_PREFIX_GROUP)) & 0xffull) ? next : run + next;
            else run = run + next;
        }
        if (g_own > 0u) {
#pragma unroll
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (!SEG || ((open >> i) & 1u)) p[i] = base + p[i];
        }
        if (SEG && (lanes & ((1ull << lane) - 1ull)) != 0ull) open = 0u;                      // a head in an earlier lane of the wave
        // level 4: the waves of a tile (run: the wave's last prefix, in every lane)
        if (lane == 0u) { wave_total[wave] = run; if (SEG) wave_head[wave] = lanes != 0ull ? 1u : 0u; }
    }
    __syncthreads();
    double run = wave_total[0];
    bool any = SEG && wave_head[0] != 0u, before = false;
#pragma unroll
    for (uint32_t w = 1; w < (uint32_t)FM_PREFIX_WAVES; ++w) {
        if (wave == w) { base = run; before = any; }
        if (SEG) { const bool h = wave_head[w] != 0u; run = h ? wave_total[w] : run + wave_total[w]; any = any || h; }
        else run = run + wave_total[w];
    }
    if (wave > 0u) {
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (!SEG || ((open >> i) & 1u)) p[i] = base + p[i];
    }
    if (SEG && before) open = 0u;                                                             // a head in an earlier wave of the tile
    // level 5: the tiles of a chunk (run: the tile's last prefix, in every thread)
    if (first_tile) carry = run;
    else {
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (!SEG || ((open >> i) & 1u)) p[i] = carry + p[i];
        if (SEG) carry = any ? run : carry + run;
        else carry = carry + run;
    }
    if (SEG) { seg.open = open; seg.any = any; }
}

// the plain tree over the lane's load
__device__ __forceinline__ void pf_tile(const PfLoad& l, const uint32_t tile, const uint32_t n, const bool first_tile, double& carry, double* wave_total, double (&p)[FM_PREFIX_ITEMS])
{
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) p[i] = e0 + (uint32_t)i < n ? (double)l.q[i >> 2][i & 3] : -0.0;
    PfSeg none{};
    pf_tile_terms<false>(first_tile, carry, wave_total, p, none, nullptr);
}

} // namespace fm
