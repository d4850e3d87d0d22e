// prefix_kernel.hip — fp64 prefix sums of a float vector for gfx950 (MI355X, CDNA4) in the nested tree of prefix_host.hpp.  DESIGN.md §4.17;
// contract: include/fmhip.h; launchers: prefix_kernel.h; engine side: prefix_engine.hpp.
//
// Three kernels chained on the stream — "totals → scan of totals → apply", as the sort's count → offsets → scatter:
//   totals   workgroup w scans ITS chunk — prefix_chunk_tiles(n) consecutive tiles — and stores { the chunk's total, the largest prefix
//            inside the chunk } with plain stores into row w of the scratch.
//   carry    ONE workgroup: the base of chunk c is the last prefix of chunk c - 1 (a serial chain over at most 1024 rows: the top level of
//            the tree), the total P[n-1]; and for a query call the chunk of every query — the position's, or the first chunk whose largest
//            prefix fl(base + largest inside) reaches the threshold.
//   apply    fmhip_prefix_sums: every workgroup scans its chunk again, adds its base and writes out[r] with 16-byte stores.
//   query    fmhip_prefix_sums_at / fmhip_prefix_search: one workgroup per query scans the located chunk up to the tile that answers it
//            and writes the prefix (and the position) into pinned memory.
// All of them scan a tile with the SAME function (pf_tile): a chunk's total is made by the operations that make its last prefix, which is
// what the monotonicity of §4.17 rests on.  -ffp-contract=off, no fast math: every fl(a + b) below is one rounded fp64 addition.
// Elements past n enter as -0.0: fl(x + (-0.0)) is x, bit for bit, for every x that is no NaN, so a unit cut short by n has the prefixes the
// definition gives it and every prefix past n repeats P[n-1].
//
// No workgroup waits for another inside a kernel: no flag, no arrival counter, no look-back; no atomics on floats, and none on global
// memory at all.  Positions are uint32 (n <= 2^31 - 1, checked by the launchers and before them by the engine); every load and store is
// bounded by n (whole quads: storage is 256-byte aligned and padded).
#include <hip/hip_runtime.h>

#include "prefix_kernel.h"
#include "prefix_device.hpp"

namespace fm {

constexpr uint32_t PF_NONE = 0xffffffffu;

// (the load of a lane's elements and the scan of a tile, pf_load and pf_tile: prefix_device.hpp)

// the larger of the two, a NaN never: NaN only while nothing else has been seen
__device__ __forceinline__ double pf_larger(const double a, const double b) { return (b > a || a != a) ? b : a; }

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_prefix_totals_kernel(const DevPrefixArgs A)
{
    __shared__ double wave_total[2][FM_PREFIX_WAVES];
    __shared__ double wave_largest[FM_PREFIX_WAVES];
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ v = reinterpret_cast<const pf_f32x4*>(A.v);
    double carry = 0.0, largest = __builtin_nan("");
    PfLoad cur = pf_load(v, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(v, tile + 1u, n);                      // in flight while this tile is scanned
        double p[FM_PREFIX_ITEMS];
        pf_tile(cur, tile, n, tile == t0, carry, wave_total[(tile - t0) & 1u], p);
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) largest = pf_larger(largest, p[i]);      // (a prefix past n repeats the last one before n)
        cur = next;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) largest = pf_larger(largest, __shfl_xor(largest, off, 64));
    if ((threadIdx.x & 63u) == 0u) wave_largest[threadIdx.x >> 6] = largest;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t w = 1; w < (uint32_t)FM_PREFIX_WAVES; ++w) largest = pf_larger(largest, wave_largest[w]);
        PrefixRow row; row.total = carry; row.largest = largest;
        prefix_rows(A)[blockIdx.x] = row;
    }
}

__global__ void __launch_bounds__(FM_PREFIX_CARRY_BLOCK) fm_prefix_carry_kernel(const DevPrefixArgs A, const uint32_t blocks)
{
    __shared__ double total[FM_PREFIX_MAX_BLOCKS], largest[FM_PREFIX_MAX_BLOCKS], base[FM_PREFIX_MAX_BLOCKS];
    __shared__ double whole;
    const PrefixRow* __restrict__ rows = prefix_rows(A);
    double* __restrict__ bases = prefix_bases(A);
    if (threadIdx.x < blocks) { const PrefixRow r = rows[threadIdx.x]; total[threadIdx.x] = r.total; largest[threadIdx.x] = r.largest; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        // level 6: the chunks of the sample
        double run = total[0];
        base[0] = 0.0;
#pragma unroll 8
        for (uint32_t c = 1; c < blocks; ++c) { base[c] = run; run = run + total[c]; }
        whole = run;
        bases[blocks] = run;
        if (A.total_host) *A.total_host = run;
    }
    __syncthreads();
    if (threadIdx.x < blocks) bases[threadIdx.x] = base[threadIdx.x];
    if (A.kind != FM_PREFIX_QUERY_NONE) {
        const uint64_t* __restrict__ queries = prefix_queries(A);
        PrefixLocated* __restrict__ located = prefix_located(A);
        const uint32_t chunk_elems = A.chunk_tiles * (uint32_t)FM_PREFIX_TILE;      // <= 2^31
        for (uint32_t j = threadIdx.x; j < A.count; j += (uint32_t)FM_PREFIX_CARRY_BLOCK) {
            PrefixLocated at; at.pad = 0u;
            if (A.kind == FM_PREFIX_QUERY_AT) {
                const uint64_t pos = queries[j];
                at.threshold = 0.0;
                at.chunk = pos < (uint64_t)A.n ? (uint32_t)pos / chunk_elems : blocks;
            } else {
                double t = __longlong_as_double((long long)queries[j]);
                if (A.relative) t = t * whole;
                // the chunk's largest prefix is fl(base + its largest inside): fl(base + x) is monotone in x.  A NaN on either side: false.
                uint32_t c = 0;
                for (; c < blocks; ++c) { const double top = c == 0u ? largest[0] : base[c] + largest[c]; if (top >= t) break; }
                at.threshold = t; at.chunk = c;
            }
            located[j] = at;
        }
    }
    __threadfence_system();
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_prefix_apply_kernel(const DevPrefixArgs A)
{
    __shared__ double wave_total[2][FM_PREFIX_WAVES];
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ v = reinterpret_cast<const pf_f32x4*>(A.v);
    pf_f32x4* __restrict__ out = reinterpret_cast<pf_f32x4*>(A.out);
    const bool first_chunk = blockIdx.x == 0u, mean = A.mode == (uint32_t)FM_PREFIX_MEAN;
    const double chunk_base = prefix_bases(A)[blockIdx.x];
    double carry = 0.0;
    PfLoad cur = pf_load(v, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(v, tile + 1u, n);
        double p[FM_PREFIX_ITEMS];
        pf_tile(cur, tile, n, tile == t0, carry, wave_total[(tile - t0) & 1u], p);
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
        pf_f32x4 o[2];
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
            const double P = first_chunk ? p[i] : chunk_base + p[i];
            o[i >> 2][i & 3] = mean ? (float)(P / (double)(e0 + (uint32_t)i + 1u)) : (float)P;
        }
        if (e0 < n) out[e0 / 4u] = o[0];                      // (storage is padded to 256 bytes: the last quad is inside it)
        if (e0 + 4u < n) out[e0 / 4u + 1u] = o[1];
        cur = next;
    }
}

// One workgroup per query: the located chunk, tile by tile, up to the tile that answers.
__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_prefix_query_kernel(const DevPrefixArgs A, const uint32_t blocks)
{
    __shared__ double wave_total[2][FM_PREFIX_WAVES];
    __shared__ uint32_t first_hit[2];
    const uint32_t n = A.n, j = blockIdx.x;
    const PrefixLocated at = prefix_located(A)[j];
    const double* __restrict__ bases = prefix_bases(A);
    const bool search = A.kind == FM_PREFIX_QUERY_SEARCH;
    if (at.chunk >= blocks) {                                 // no prefix reaches the threshold: n and P[n-1]
        if (threadIdx.x == 0u) { A.sums_host[j] = bases[blocks]; if (search) A.positions_host[j] = (uint64_t)n; }
        __threadfence_system();
        return;
    }
    if (threadIdx.x < 2u) first_hit[threadIdx.x] = PF_NONE;
    __syncthreads();
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = at.chunk * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ v = reinterpret_cast<const pf_f32x4*>(A.v);
    const bool first_chunk = at.chunk == 0u;
    const double chunk_base = bases[at.chunk], t = at.threshold;
    const uint32_t pos = search ? 0u : (uint32_t)prefix_queries(A)[j];           // < n: the carry kernel has looked
    double carry = 0.0;
    bool answered = false;
    PfLoad cur = pf_load(v, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1 && !answered; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(v, tile + 1u, n);
        double p[FM_PREFIX_ITEMS];
        pf_tile(cur, tile, n, tile == t0, carry, wave_total[(tile - t0) & 1u], p);
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
        uint32_t own = PF_NONE;                               // the lane's element that answers
        double own_sum = 0.0;
#pragma unroll
        for (int i = FM_PREFIX_ITEMS - 1; i >= 0; --i) {
            const double P = first_chunk ? p[i] : chunk_base + p[i];
            const uint32_t e = e0 + (uint32_t)i;
            if (search ? (e < n && P >= t) : e == pos) { own = e; own_sum = P; }
        }
        if (search) {
            uint32_t* const slot = &first_hit[(tile - t0) & 1u];              // (the other slot is still PF_NONE: a tile with a hit is the last)
            if (own != PF_NONE) atomicMin(slot, own);
            __syncthreads();
            const uint32_t hit = *slot;
            answered = hit != PF_NONE;
            if (answered && own == hit) { A.sums_host[j] = own_sum; A.positions_host[j] = (uint64_t)hit; }
        } else {
            answered = pos / (uint32_t)FM_PREFIX_TILE == tile;
            if (own != PF_NONE) A.sums_host[j] = own_sum;
        }
        cur = next;
    }
    if (!answered && threadIdx.x == 0u) { A.sums_host[j] = bases[blocks]; if (search) A.positions_host[j] = (uint64_t)n; }
    __threadfence_system();
}

hipError_t launch_prefix_sums(const DevPrefixArgs& a, hipStream_t st)
{
    if (!prefix_shape_ok(a) || a.kind != FM_PREFIX_QUERY_NONE) return hipErrorInvalidValue;
    const uint32_t blocks = prefix_blocks((int64_t)a.n);
    hipLaunchKernelGGL(fm_prefix_totals_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_prefix_carry_kernel, dim3(1), dim3(FM_PREFIX_CARRY_BLOCK), 0, st, a, blocks);
    hipLaunchKernelGGL(fm_prefix_apply_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_prefix_queries(const DevPrefixArgs& a, hipStream_t st)
{
    if (!prefix_shape_ok(a) || a.kind == FM_PREFIX_QUERY_NONE) return hipErrorInvalidValue;
    const uint32_t blocks = prefix_blocks((int64_t)a.n);
    hipLaunchKernelGGL(fm_prefix_totals_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_prefix_carry_kernel, dim3(1), dim3(FM_PREFIX_CARRY_BLOCK), 0, st, a, blocks);
    hipLaunchKernelGGL(fm_prefix_query_kernel, dim3(a.count), dim3(FM_PREFIX_BLOCK), 0, st, a, blocks);
    return hipGetLastError();
}

} // namespace fm
