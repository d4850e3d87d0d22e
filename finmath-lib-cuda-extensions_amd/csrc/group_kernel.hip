// group_kernel.hip — reduce by key for gfx950 (MI355X, CDNA4): count, sum, mean and variance per group of an index vector.  DESIGN.md
// §4.29; contract: include/fmhip.h; launchers: group_kernel.h; engine side: group_engine.hpp; the definition, and every function of it
// called below (group_key, group_output): group_host.hpp, compiled here as it is compiled for the host.
//
//   keys     one streaming kernel: key[j] = group_key(index[j], m) — the group, or m for an element that belongs to none — and idx[j] = j.
//            Every later address comes from this checked key.
//   (order)  the radix sort's passes over that pair (sort_kernel.hip, launch_sort_pass with from_floats = 0): one for m <= 255, two up to 65 535, three below
//            2^24 and four at m = 2^24 — the keys are 0 … m inclusive.
//   fill     the outputs take the empty-group values: count 0, sum +0.0, mean and variance NaN.
//   totals   workgroup w scans ITS chunk of the sorted sequence — the chunks of the prefix passes (prefix_host.hpp) — and stores the chunk's
//            last run-prefix of S1 and S2 and its last head position.
//   carry    ONE workgroup: the base of chunk c is the last run-prefix of chunk c - 1 — the serial chain of the definition, which a chunk
//            with a head cuts — and the last head position before the chunk.
//   apply    every workgroup scans its chunk again and, at every run tail with key < m, stores the count and the masked outputs at [key].
// totals and apply scan a tile with the tile scan of the prefix passes extended by the head flags (pf_tile_terms<true>, prefix_device.hpp):
// the run-prefixes are the definition's, bit for bit.  The count of a run is its tail position minus its head position plus one: an integer
// max-scan of the head positions beside the sums.
//
// No workgroup waits for another; no atomics; positions are uint32 (n <= 2^31 - 1).  Every address is checked against its bound before the
// access: a sorted position against n (whole quads: storage is 256-byte aligned and padded), a path index clamped into [0, n - 1] before it
// reads a value, a key compared with m before it addresses an output.
#include <hip/hip_runtime.h>

#include "group_kernel.h"
#include "prefix_device.hpp"

namespace fm {

typedef uint32_t gr_u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(FM_GROUP_BLOCK) fm_group_keys_kernel(const DevGroupKeysArgs A)
{
    const float* __restrict__ index = reinterpret_cast<const float*>(A.index);
    uint32_t* __restrict__ key = reinterpret_cast<uint32_t*>(A.key_out);
    uint32_t* __restrict__ idx = reinterpret_cast<uint32_t*>(A.idx_out);
    const uint64_t n = A.n, stride = (uint64_t)gridDim.x * FM_GROUP_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * FM_GROUP_BLOCK + threadIdx.x; j < n; j += stride) {
        key[j] = group_key(index[j], (int64_t)A.m);
        idx[j] = (uint32_t)j;
    }
}

__global__ void __launch_bounds__(FM_GROUP_BLOCK) fm_group_fill_kernel(const DevGroupScanArgs A)
{
    float* __restrict__ counts = reinterpret_cast<float*>(A.counts_out);
    const uint64_t m = A.m, stride = (uint64_t)gridDim.x * FM_GROUP_BLOCK;
    for (uint64_t k = (uint64_t)blockIdx.x * FM_GROUP_BLOCK + threadIdx.x; k < m; k += stride) {
        if (counts) counts[k] = 0.0f;
        int j = 0;
#pragma unroll
        for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1)
            if (A.mask & (uint32_t)bit) reinterpret_cast<float*>(A.outs[j++])[k] = group_output(bit, 0.0, 0.0, 0);
    }
}

// the lane's 8 consecutive words of `tile`: two 16-byte loads (pf_load for uint32)
__device__ __forceinline__ void gr_load(const gr_u32x4* __restrict__ v, const uint32_t tile, const uint32_t n, uint32_t (&x)[FM_PREFIX_ITEMS])
{
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
    const gr_u32x4 a = v[e0 < n ? e0 / 4u : 0u], b = v[e0 + 4u < n ? e0 / 4u + 1u : 0u];
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[i] = a[i]; x[4 + i] = b[i]; }
}

// One tile of the sorted sequence in a lane: its keys, which of its elements start and end a run, the last head position + 1 at or before
// each element (start), the run-prefixes inside the chunk (p1, p2) and which of them the chunk's base is still to be added to (open).
struct GrTile {
    uint32_t key[FM_PREFIX_ITEMS], start[FM_PREFIX_ITEMS];
    uint32_t heads, tails, open;
    double p1[FM_PREFIX_ITEMS], p2[FM_PREFIX_ITEMS];
};
// the state a workgroup carries from tile to tile of its chunk
struct GrChunk {
    double carry1 = 0.0, carry2 = 0.0;
    uint32_t start = 0u;       // the last head position + 1 so far (apply: from the chunk's base)
    bool open = true;          // no head in the chunk so far
};
struct GrShared {
    double wave_total[2][2][FM_PREFIX_WAVES];
    uint32_t wave_head[2][2][FM_PREFIX_WAVES];
    uint32_t wave_start[2][FM_PREFIX_WAVES];
};

template <int MODE>
__device__ __forceinline__ void gr_tile(const DevGroupScanArgs& A, const uint32_t tile, const bool first_tile, const uint32_t parity, GrShared& sh, GrChunk& c, GrTile& t)
{
    const uint32_t n = A.n, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
    const uint32_t* __restrict__ key = reinterpret_cast<const uint32_t*>(A.key);
    gr_load(reinterpret_cast<const gr_u32x4*>(A.key), tile, n, t.key);
    const uint32_t before = e0 > 0u && e0 < n ? key[e0 - 1u] : 0u, behind = e0 + (uint32_t)FM_PREFIX_ITEMS < n ? key[e0 + (uint32_t)FM_PREFIX_ITEMS] : 0u;
    t.heads = 0u; t.tails = 0u;
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
        const uint32_t r = e0 + (uint32_t)i;
        if (r < n) {
            if (r == 0u || t.key[i] != (i == 0 ? before : t.key[i > 0 ? i - 1 : 0])) t.heads |= 1u << i;
            if (r == n - 1u || t.key[i] != (i == FM_PREFIX_ITEMS - 1 ? behind : t.key[i < FM_PREFIX_ITEMS - 1 ? i + 1 : i])) t.tails |= 1u << i;
        }
    }
    // the head positions: a max-scan along the lane, over the lanes of the wave, over the waves of the tile, over the tiles of the chunk
    uint32_t own = 0u;
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) { if ((t.heads >> i) & 1u) own = e0 + (uint32_t)i + 1u; t.start[i] = own; }
    uint32_t inclusive = own;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)inclusive, d, 64);
        if (lane >= d && below > inclusive) inclusive = below;
    }
    uint32_t earlier = (uint32_t)__shfl_up((int)inclusive, 1u, 64);
    if (lane == 0u) earlier = 0u;
    if (lane == 63u) sh.wave_start[parity][wave] = inclusive;
    if (MODE != FM_GROUP_COUNTS) {
        const uint32_t* __restrict__ perm = reinterpret_cast<const uint32_t*>(A.perm);
        const float* __restrict__ values = reinterpret_cast<const float*>(A.values);
        uint32_t at[FM_PREFIX_ITEMS];
        gr_load(reinterpret_cast<const gr_u32x4*>(perm), tile, n, at);
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
            const float x = values[at[i] < n ? at[i] : n - 1u];                       // (an element past n reads a valid one and drops it)
            t.p1[i] = e0 + (uint32_t)i < n ? (double)x : -0.0;
            if (MODE == FM_GROUP_S1_S2) t.p2[i] = e0 + (uint32_t)i < n ? (double)x * (double)x : -0.0;
        }
        PfSeg seg; seg.heads = t.heads; seg.open = 0u; seg.any = false;
        pf_tile_terms<true>(first_tile, c.carry1, sh.wave_total[parity][0], t.p1, seg, sh.wave_head[parity][0]);      // (its barrier covers wave_start)
        if (MODE == FM_GROUP_S1_S2) pf_tile_terms<true>(first_tile, c.carry2, sh.wave_total[parity][1], t.p2, seg, sh.wave_head[parity][1]);
        t.open = c.open ? seg.open : 0u;
        c.open = c.open && !seg.any;
    } else {
        t.open = 0u;
        __syncthreads();
    }
    uint32_t tile_start = 0u;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)FM_PREFIX_WAVES; ++w) {
        const uint32_t s = sh.wave_start[parity][w];
        if (w < wave && s > earlier) earlier = s;
        if (s > tile_start) tile_start = s;
    }
    if (c.start > earlier) earlier = c.start;
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (earlier > t.start[i]) t.start[i] = earlier;
    if (tile_start > c.start) c.start = tile_start;
}

template <int MODE>
__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_group_totals_kernel(const DevGroupScanArgs A)
{
    __shared__ GrShared sh;
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    GrChunk c;
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        GrTile t;
        gr_tile<MODE>(A, tile, tile == t0, (tile - t0) & 1u, sh, c, t);
    }
    if (threadIdx.x == 0u) {
        GroupRow row; row.s1 = c.carry1; row.s2 = c.carry2; row.head = c.start; row.pad = 0u;
        group_rows(A)[blockIdx.x] = row;
    }
}

__global__ void __launch_bounds__(FM_PREFIX_CARRY_BLOCK) fm_group_carry_kernel(const DevGroupScanArgs A, const uint32_t blocks)
{
    __shared__ double s1[FM_PREFIX_MAX_BLOCKS], s2[FM_PREFIX_MAX_BLOCKS];
    __shared__ uint32_t head[FM_PREFIX_MAX_BLOCKS];
    const GroupRow* __restrict__ rows = group_rows(A);
    GroupRow* __restrict__ bases = group_bases(A);
    if (threadIdx.x < blocks) { const GroupRow r = rows[threadIdx.x]; s1[threadIdx.x] = r.s1; s2[threadIdx.x] = r.s2; head[threadIdx.x] = r.head; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        // level 6: the chunks of the sample.  Entry c leaves as the base of chunk c (the first chunk takes none).
        double run1 = s1[0], run2 = s2[0];
        uint32_t start = head[0];
        s1[0] = 0.0; s2[0] = 0.0; head[0] = 0u;
#pragma unroll 4
        for (uint32_t c = 1; c < blocks; ++c) {
            const double a = s1[c], b = s2[c];
            const uint32_t h = head[c];
            s1[c] = run1; s2[c] = run2; head[c] = start;
            run1 = h != 0u ? a : run1 + a;
            run2 = h != 0u ? b : run2 + b;
            if (h > start) start = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < blocks) { GroupRow r; r.s1 = s1[threadIdx.x]; r.s2 = s2[threadIdx.x]; r.head = head[threadIdx.x]; r.pad = 0u; bases[threadIdx.x] = r; }
}

template <int MODE>
__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_group_apply_kernel(const DevGroupScanArgs A)
{
    __shared__ GrShared sh;
    const uint32_t n = A.n, m = A.m;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const bool first_chunk = blockIdx.x == 0u;
    const GroupRow base = group_bases(A)[blockIdx.x];
    float* __restrict__ counts = reinterpret_cast<float*>(A.counts_out);
    GrChunk c;
    c.start = base.head;
    uint64_t ungrouped = ~uint64_t(0);                        // set in ONE lane of the grid: the head of the run of key m, or the tail at n - 1 where there is none
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        GrTile t;
        gr_tile<MODE>(A, tile, tile == t0, (tile - t0) & 1u, sh, c, t);
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
            const uint32_t r = e0 + (uint32_t)i, k = t.key[i];
            if (((t.heads >> i) & 1u) && k >= m) ungrouped = (uint64_t)(n - r);
            if (!((t.tails >> i) & 1u) || k >= m) continue;
            if (r == n - 1u) ungrouped = 0u;
            const int64_t count = (int64_t)r + 2 - (int64_t)t.start[i];              // (start >= 1: position 0 is a head)
            if (counts) counts[k] = (float)count;
            if (MODE != FM_GROUP_COUNTS) {
                const bool add = !first_chunk && ((t.open >> i) & 1u);
                const double S1 = add ? base.s1 + t.p1[i] : t.p1[i];
                double S2 = 0.0;
                if (MODE == FM_GROUP_S1_S2) S2 = add ? base.s2 + t.p2[i] : t.p2[i];
                int j = 0;
#pragma unroll
                for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1)
                    if (A.mask & (uint32_t)bit) reinterpret_cast<float*>(A.outs[j++])[k] = group_output(bit, S1, S2, count);
            }
        }
    }
    if (A.ungrouped_host && ungrouped != ~uint64_t(0)) { *A.ungrouped_host = ungrouped; __threadfence_system(); }
}

static uint32_t gr_stream_blocks(uint64_t elements)
{
    const uint64_t b = (elements + FM_GROUP_BLOCK - 1) / FM_GROUP_BLOCK;
    return (uint32_t)(b < 1u ? 1u : b > (uint64_t)FM_GROUP_STREAM_MAX_BLOCKS ? (uint64_t)FM_GROUP_STREAM_MAX_BLOCKS : b);
}

hipError_t launch_group_keys(const DevGroupKeysArgs& a, hipStream_t st)
{
    if (!group_keys_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_group_keys_kernel, dim3(gr_stream_blocks(a.n)), dim3(FM_GROUP_BLOCK), 0, st, a);
    return hipGetLastError();
}

template <int MODE>
static void gr_launch_scan(const DevGroupScanArgs& a, const uint32_t blocks, hipStream_t st)
{
    hipLaunchKernelGGL(fm_group_totals_kernel<MODE>, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_group_carry_kernel, dim3(1), dim3(FM_PREFIX_CARRY_BLOCK), 0, st, a, blocks);
    hipLaunchKernelGGL(fm_group_apply_kernel<MODE>, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
}

hipError_t launch_group_scan(const DevGroupScanArgs& a, hipStream_t st)
{
    if (!group_scan_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t blocks = prefix_blocks((int64_t)a.n);
    if (a.counts_out || a.mask) hipLaunchKernelGGL(fm_group_fill_kernel, dim3(gr_stream_blocks(a.m)), dim3(FM_GROUP_BLOCK), 0, st, a);
    if (a.mode == (uint32_t)FM_GROUP_COUNTS) gr_launch_scan<FM_GROUP_COUNTS>(a, blocks, st);
    else if (a.mode == (uint32_t)FM_GROUP_S1) gr_launch_scan<FM_GROUP_S1>(a, blocks, st);
    else gr_launch_scan<FM_GROUP_S1_S2>(a, blocks, st);
    return hipGetLastError();
}

} // namespace fm
