// resample_kernel.hip — resampling for gfx950 (MI355X, CDNA4): m ancestors drawn from n weights, up to 8 companion vectors gathered along.
// DESIGN.md §4.26; contract: include/fmhip.h; launcher: resample_kernel.h; engine side: resample_engine.hpp; the definition, and every
// function of it called below (resample_clean, resample_uniform, resample_fraction, resample_target, resample_search_step …):
// resample_host.hpp, compiled here as it is compiled for the host — the ancestors are the host's bit for bit.
//
// A weighted call is four kernels chained on the stream, the first three in the shape of prefix_kernel.hip (whose tile scan, pf_tile of
// prefix_device.hpp, they share: P is made by the operations that make fmhip_prefix_sums_host's):
//   totals    workgroup w scans ITS chunk of the CLEANED weights (cleaned in the load) and stores the chunk's total.
//   carry     ONE workgroup: the base of chunk c is the last prefix of chunk c - 1; the total P[n-1], also into pinned memory.
//   prefixes  every workgroup scans its chunk again, adds its base and writes P[r] in fp64 into the temporary (8n bytes, 16-byte stores).
//   gather    FM_RESAMPLE_ITEMS outputs per lane, FM_RESAMPLE_BLOCK apart.  The table of the chunks' last prefixes (bases[c + 1], at most
//             1024 doubles) sits in LDS; a lane bisects it for the chunk of t_j, then bisects P inside the chunk, clamps the index into
//             [0, n-1] and loads the companions; stores are coalesced.  The steps of a lane's outputs run side by side: their loads are in
//             flight together.
// With equal weights the gather runs alone: no prefix, no table, no search.
//
// Every bisection runs a trip count that the launcher derives from n (the bit lengths of the number of chunks and of a chunk): no loop
// depends on data, and every load address is clamped before the load — NaN weights, uniforms outside [0, 1) or a zero total cannot make a
// lane read out of bounds or loop without bound.  No atomics, no workgroup waits for another, no scratch (private segment 0 in every
// instantiation), no host round trip between the launches.
//
// Shaped for ASCENDING targets (systematic, stratified): neighbouring lanes bisect to neighbouring prefixes, the last steps of a wave fall
// into a few cache lines and the companions' loads are nearly coalesced.  Multinomial targets are random 8-byte and 4-byte reads: the same
// code, priced by DESIGN.md §4.26.
#include <hip/hip_runtime.h>

#include "resample_kernel.h"
#include "prefix_device.hpp"

namespace fm {

typedef double rs_f64x2 __attribute__((ext_vector_type(2)));

// the lane's 8 consecutive CLEANED weights of `tile`
__device__ __forceinline__ PfLoad rs_load(const pf_f32x4* __restrict__ w, const uint32_t tile, const uint32_t n)
{
    PfLoad l = pf_load(w, tile, n);
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) l.q[i >> 2][i & 3] = resample_clean(l.q[i >> 2][i & 3]);
    return l;
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_resample_totals_kernel(const DevResampleArgs A)
{
    __shared__ double wave_total[2][FM_PREFIX_WAVES];
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ w = reinterpret_cast<const pf_f32x4*>(A.weights);
    double carry = 0.0;
    PfLoad cur = rs_load(w, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = rs_load(w, tile + 1u, n);                      // in flight while this tile is scanned
        double p[FM_PREFIX_ITEMS];
        pf_tile(cur, tile, n, tile == t0, carry, wave_total[(tile - t0) & 1u], p);
        cur = next;
    }
    if (threadIdx.x == 0u) resample_totals(A)[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(FM_PREFIX_CARRY_BLOCK) fm_resample_carry_kernel(const DevResampleArgs A, const uint32_t blocks)
{
    __shared__ double total[FM_PREFIX_MAX_BLOCKS], base[FM_PREFIX_MAX_BLOCKS];
    const double* __restrict__ totals = resample_totals(A);
    double* __restrict__ bases = resample_bases(A);
    if (threadIdx.x < blocks) total[threadIdx.x] = totals[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0u) {
        // level 6: the chunks of the sample
        double run = total[0];
        base[0] = 0.0;
#pragma unroll 8
        for (uint32_t c = 1; c < blocks; ++c) { base[c] = run; run = run + total[c]; }
        bases[blocks] = run;
        if (A.total_host) *A.total_host = run;
    }
    __syncthreads();
    if (threadIdx.x < blocks) bases[threadIdx.x] = base[threadIdx.x];
    __threadfence_system();
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_resample_prefix_kernel(const DevResampleArgs A)
{
    __shared__ double wave_total[2][FM_PREFIX_WAVES];
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ w = reinterpret_cast<const pf_f32x4*>(A.weights);
    double* __restrict__ P = A.prefix;
    const bool first_chunk = blockIdx.x == 0u;
    const double chunk_base = resample_bases(A)[blockIdx.x];
    double carry = 0.0;
    PfLoad cur = rs_load(w, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = rs_load(w, tile + 1u, n);
        double p[FM_PREFIX_ITEMS];
        pf_tile(cur, tile, n, tile == t0, carry, wave_total[(tile - t0) & 1u], p);
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
#pragma unroll
        for (int i = 0; i < FM_PREFIX_ITEMS; i += 2) {
            rs_f64x2 o;
            o[0] = first_chunk ? p[i] : chunk_base + p[i];
            o[1] = first_chunk ? p[i + 1] : chunk_base + p[i + 1];
            const uint32_t e = e0 + (uint32_t)i;                                 // even: 16-byte aligned in a 256-byte aligned buffer
            if (e + 1u < n) *reinterpret_cast<rs_f64x2*>(P + e) = o;
            else if (e < n) P[e] = o[0];
        }
        cur = next;
    }
}

template <bool WEIGHTED>
__global__ void __launch_bounds__(FM_RESAMPLE_BLOCK) fm_resample_gather_kernel(const DevResampleArgs A, const uint32_t blocks, const int chunk_trips, const int inner_trips)
{
    __shared__ double tops[WEIGHTED ? FM_PREFIX_MAX_BLOCKS : 1];       // tops[c]: the last prefix of chunk c
    const int64_t n = (int64_t)A.n, m = (int64_t)A.m;
    double total = (double)n;
    if (WEIGHTED) {
        const double* __restrict__ bases = resample_bases(A);
        for (uint32_t c = threadIdx.x; c < blocks; c += (uint32_t)FM_RESAMPLE_BLOCK) tops[c] = bases[c + 1u];
        total = bases[blocks];
        __syncthreads();
    }
    const bool degenerate = resample_degenerate(total);
    const int scheme = (int)A.scheme;
    const float* __restrict__ uniforms = reinterpret_cast<const float*>(A.uniforms);
    const int64_t j0 = (int64_t)blockIdx.x * FM_RESAMPLE_TILE + (int64_t)threadIdx.x;
    double t[FM_RESAMPLE_ITEMS];
    bool alive[FM_RESAMPLE_ITEMS];
    int64_t a[FM_RESAMPLE_ITEMS];
#pragma unroll
    for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) {
        const int64_t j = j0 + (int64_t)k * FM_RESAMPLE_BLOCK;
        double U = 0.0;
        alive[k] = j < m && !degenerate;
        if (alive[k] && resample_needs_uniforms(scheme)) alive[k] = resample_uniform(uniforms[j], U);
        t[k] = alive[k] ? resample_target(resample_fraction(scheme, j, m, A.offset, U), total) : 0.0;
    }
    if (WEIGHTED) {
        const int64_t chunk_elems = (int64_t)A.chunk_tiles * FM_PREFIX_TILE;
        int64_t lo[FM_RESAMPLE_ITEMS], len[FM_RESAMPLE_ITEMS];
#pragma unroll
        for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) { lo[k] = 0; len[k] = (int64_t)blocks; }
        for (int it = 0; it < chunk_trips; ++it) {
#pragma unroll
            for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) resample_search_step(tops, lo[k], len[k], (int64_t)blocks - 1, t[k], total);
        }
#pragma unroll
        for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) {
            const int64_t c = lo[k] < (int64_t)blocks - 1 ? lo[k] : (int64_t)blocks - 1;       // (the last chunk's last prefix IS the total: lo < blocks)
            lo[k] = c * chunk_elems;
            len[k] = n - lo[k] < chunk_elems ? n - lo[k] : chunk_elems;
        }
        const double* __restrict__ P = A.prefix;
        for (int it = 0; it < inner_trips; ++it) {
#pragma unroll
            for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) resample_search_step(P, lo[k], len[k], n - 1, t[k], total);
        }
#pragma unroll
        for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) a[k] = lo[k];
    } else {
#pragma unroll
        for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) a[k] = resample_equal_ancestor(t[k], n);
    }
#pragma unroll
    for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) a[k] = a[k] < 0 ? 0 : a[k] > n - 1 ? n - 1 : a[k];      // the clamp before every load below
    if (A.ancestors_out) {
        uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.ancestors_out);
#pragma unroll
        for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) {
            const int64_t j = j0 + (int64_t)k * FM_RESAMPLE_BLOCK;
            if (j < m) out[j] = alive[k] ? __float_as_uint((float)a[k]) : FM_RESAMPLE_NAN_BITS;
        }
    }
#pragma unroll
    for (int i = 0; i < FM_RESAMPLE_MAX_VALUES; ++i) {
        if ((uint32_t)i < A.n_values) {
            const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(A.values[i]);
            uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.values_out[i]);
            uint32_t x[FM_RESAMPLE_ITEMS];
#pragma unroll
            for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) x[k] = src[a[k]];                      // (a dead lane reads a valid element and drops it)
#pragma unroll
            for (int k = 0; k < FM_RESAMPLE_ITEMS; ++k) {
                const int64_t j = j0 + (int64_t)k * FM_RESAMPLE_BLOCK;
                if (j < m) out[j] = alive[k] ? x[k] : FM_RESAMPLE_NAN_BITS;
            }
        }
    }
}

hipError_t launch_resample(const DevResampleArgs& a, hipStream_t st)
{
    if (!resample_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((int64_t)a.m + FM_RESAMPLE_TILE - 1) / FM_RESAMPLE_TILE);
    if (!a.weights) {
        hipLaunchKernelGGL(fm_resample_gather_kernel<false>, dim3(grid), dim3(FM_RESAMPLE_BLOCK), 0, st, a, 0u, 0, 0);
        return hipGetLastError();
    }
    const int64_t n = (int64_t)a.n;
    const uint32_t blocks = prefix_blocks(n);
    const int64_t chunk = prefix_chunk_elems(n) < n ? prefix_chunk_elems(n) : n;
    hipLaunchKernelGGL(fm_resample_totals_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_resample_carry_kernel, dim3(1), dim3(FM_PREFIX_CARRY_BLOCK), 0, st, a, blocks);
    hipLaunchKernelGGL(fm_resample_prefix_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_resample_gather_kernel<true>, dim3(grid), dim3(FM_RESAMPLE_BLOCK), 0, st, a, blocks, resample_trips((int64_t)blocks), resample_trips(chunk));
    return hipGetLastError();
}

} // namespace fm
