// select_kernel.hip — selection for gfx950 (MI355X, CDNA4): the paths on which a mask is selected, compressed into shorter vectors, expanded
// back, and the gather by a caller's index.  DESIGN.md §4.27; contract: include/fmhip.h; launchers: select_kernel.h; engine side:
// select_engine.hpp; the definition, and every function of it called below (select_selected, select_index): select_host.hpp, compiled here
// as it is compiled for the host.  Counts are integers: nothing below depends on an order of summation, the bits are the host twins'.
//
// The chunks and tiles are the prefix passes' (prefix_host.hpp; pf_load of prefix_device.hpp): workgroup w owns the tiles of chunk w, a lane
// eight consecutive elements of a tile, which it turns into eight bits.
//   count     workgroup w counts the selected elements of ITS chunk (popcounts, an integer shuffle reduce, four wave totals in LDS) and
//             stores the count as uint32.
//   carry     ONE workgroup: the chunk counts become exclusive bases; the count of the mask goes to pinned memory.  The flag is raised
//             behind it, the host reads the count and allocates outputs of exactly that size — the one extra wait of §4.27.
//   compress  every workgroup reads its chunk's mask again, rebuilds the bits and scans them inside the tile — lane popcount, a wave scan by
//             shuffles, the wave totals in LDS, the tile's running base, the chunk base — and stores the selected elements of every value
//             vector, and the positions, at base + q.  The stores go straight to memory: those of a wave fall into one ascending run.
//   expand    the same scan; element r of an output is values[base + q] where it is selected, the fill otherwise; 16-byte stores.
//   gather    FM_SELECT_ITEMS outputs per lane, FM_SELECT_BLOCK apart, in the shape of the resampling's gather with equal weights: the
//             index is decoded by select_index, clamped, the loads of a lane's outputs are in flight together, the stores are coalesced.
//
// Every loop's trip count is a function of n alone.  Every address is checked against its bound before the access: a store of the compress
// against the count the host allocated (dst < count), a load of the expand clamped into [0, count - 1], a load of the gather clamped into
// [0, n - 1] — a wrong count, a NaN mask or a hostile index cannot make a lane touch memory outside its vectors.  No atomics, no workgroup
// waits for another, no scratch (private segment 0 in every kernel).
#include <hip/hip_runtime.h>

#include "select_kernel.h"
#include "prefix_device.hpp"

namespace fm {

// the lane's eight elements of the mask as bits: bit i is set where element e0 + i exists and is selected
__device__ __forceinline__ uint32_t sl_bits(const PfLoad& l, const uint32_t tile, const uint32_t n)
{
    const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
    uint32_t bits = 0u;
#pragma unroll
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i)
        if (e0 + (uint32_t)i < n && select_selected(l.q[i >> 2][i & 3])) bits |= 1u << i;
    return bits;
}

// The number of selected elements of the tile before the lane's, and the tile's total (in every thread).  wave_total: four words of LDS,
// written again two tiles later.  Every thread of the workgroup calls (one barrier).
__device__ __forceinline__ uint32_t sl_tile_scan(const uint32_t own, uint32_t* wave_total, uint32_t& tile_total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inclusive = own;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)inclusive, d, 64);
        if (lane >= d) inclusive += below;
    }
    if (lane == 63u) wave_total[wave] = inclusive;
    __syncthreads();
    uint32_t before = inclusive - own, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)FM_PREFIX_WAVES; ++w) {
        const uint32_t t = wave_total[w];
        if (w < wave) before += t;
        total += t;
    }
    tile_total = total;
    return before;
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_select_count_kernel(const DevCompressArgs A)
{
    __shared__ uint32_t wave_count[FM_PREFIX_WAVES];
    const uint32_t n = A.n;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ mask = reinterpret_cast<const pf_f32x4*>(A.mask);
    uint32_t own = 0u;
    PfLoad cur = pf_load(mask, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(mask, tile + 1u, n);                    // in flight while this tile is counted
        own += (uint32_t)__popc(sl_bits(cur, tile, n));
        cur = next;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) own += (uint32_t)__shfl_xor((int)own, d, 64);
    if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = own;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t c = 0u;
#pragma unroll
        for (int w = 0; w < FM_PREFIX_WAVES; ++w) c += wave_count[w];
        select_counts(A)[blockIdx.x] = c;
    }
}

__global__ void __launch_bounds__(FM_PREFIX_CARRY_BLOCK) fm_select_carry_kernel(const DevCompressArgs A, const uint32_t blocks)
{
    __shared__ uint32_t count[FM_PREFIX_MAX_BLOCKS], base[FM_PREFIX_MAX_BLOCKS];
    const uint32_t* __restrict__ counts = select_counts(A);
    uint32_t* __restrict__ bases = select_bases(A);
    if (threadIdx.x < blocks) count[threadIdx.x] = counts[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t run = 0u;
#pragma unroll 8
        for (uint32_t c = 0; c < blocks; ++c) { base[c] = run; run += count[c]; }
        bases[blocks] = run;
        *A.count_host = (uint64_t)run;
    }
    __syncthreads();
    if (threadIdx.x < blocks) bases[threadIdx.x] = base[threadIdx.x];
    __threadfence_system();
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_select_compress_kernel(const DevCompressArgs A)
{
    __shared__ uint32_t wave_total[2][FM_PREFIX_WAVES];
    const uint32_t n = A.n, count = A.count;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ mask = reinterpret_cast<const pf_f32x4*>(A.mask);
    uint32_t* __restrict__ positions = reinterpret_cast<uint32_t*>(A.positions_out);
    uint32_t run = select_bases(A)[blockIdx.x];                                     // the selected elements before this tile
    PfLoad cur = pf_load(mask, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(mask, tile + 1u, n);
        const uint32_t bits = sl_bits(cur, tile, n);
        uint32_t tile_total;
        const uint32_t q0 = run + sl_tile_scan((uint32_t)__popc(bits), wave_total[(tile - t0) & 1u], tile_total);
        run += tile_total;
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
        if (positions) {
#pragma unroll
            for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
                const uint32_t dst = q0 + (uint32_t)__popc(bits & ((1u << i) - 1u));
                if ((bits >> i & 1u) && dst < count) positions[dst] = __float_as_uint((float)(e0 + (uint32_t)i));
            }
        }
#pragma unroll
        for (int v = 0; v < FM_SELECT_MAX_VALUES; ++v) {
            if ((uint32_t)v < A.n_values) {
                const PfLoad x = pf_load(reinterpret_cast<const pf_f32x4*>(A.values[v]), tile, n);
                uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.values_out[v]);
#pragma unroll
                for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
                    const uint32_t dst = q0 + (uint32_t)__popc(bits & ((1u << i) - 1u));
                    if ((bits >> i & 1u) && dst < count) out[dst] = __float_as_uint(x.q[i >> 2][i & 3]);
                }
            }
        }
        cur = next;
    }
}

__global__ void __launch_bounds__(FM_PREFIX_BLOCK) fm_select_expand_kernel(const DevCompressArgs A)
{
    __shared__ uint32_t wave_total[2][FM_PREFIX_WAVES];
    const uint32_t n = A.n, last = A.count - 1u;                                    // (count >= 1: select_shape_ok)
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_PREFIX_TILE - 1) / FM_PREFIX_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const pf_f32x4* __restrict__ mask = reinterpret_cast<const pf_f32x4*>(A.mask);
    const uint32_t fill = __float_as_uint(A.fill);
    uint32_t run = select_bases(A)[blockIdx.x];
    PfLoad cur = pf_load(mask, t0 < tiles ? t0 : 0u, n);
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        PfLoad next = cur;
        if (tile + 1u < t1) next = pf_load(mask, tile + 1u, n);
        const uint32_t bits = sl_bits(cur, tile, n);
        uint32_t tile_total;
        const uint32_t q0 = run + sl_tile_scan((uint32_t)__popc(bits), wave_total[(tile - t0) & 1u], tile_total);
        run += tile_total;
        const uint32_t e0 = tile * (uint32_t)FM_PREFIX_TILE + threadIdx.x * (uint32_t)FM_PREFIX_ITEMS;
#pragma unroll
        for (int v = 0; v < FM_SELECT_MAX_VALUES; ++v) {
            if ((uint32_t)v < A.n_values) {
                const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(A.values[v]);
                uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.values_out[v]);
                uint32_t x[FM_PREFIX_ITEMS];
#pragma unroll
                for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
                    const uint32_t q = q0 + (uint32_t)__popc(bits & ((1u << i) - 1u));
                    x[i] = src[q < last ? q : last];                                // (an element that is not selected reads a valid one and drops it)
                }
#pragma unroll
                for (int i = 0; i < FM_PREFIX_ITEMS; ++i) x[i] = (bits >> i & 1u) ? x[i] : fill;
#pragma unroll
                for (int h = 0; h < FM_PREFIX_ITEMS; h += 4) {
                    const uint32_t e = e0 + (uint32_t)h;                             // a multiple of 4: 16-byte aligned in a 256-byte aligned buffer
                    if (e + 3u < n) {
                        uint4 o; o.x = x[h]; o.y = x[h + 1]; o.z = x[h + 2]; o.w = x[h + 3];
                        *reinterpret_cast<uint4*>(out + e) = o;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) if (e + (uint32_t)i < n) out[e + (uint32_t)i] = x[h + i];
                    }
                }
            }
        }
        cur = next;
    }
}

__global__ void __launch_bounds__(FM_SELECT_BLOCK) fm_select_gather_kernel(const DevIndexGatherArgs A)
{
    const int64_t n = (int64_t)A.n, m = (int64_t)A.m;
    const float* __restrict__ index = reinterpret_cast<const float*>(A.index);
    const int64_t j0 = (int64_t)blockIdx.x * FM_SELECT_TILE + (int64_t)threadIdx.x;
    bool alive[FM_SELECT_ITEMS];
    int64_t k[FM_SELECT_ITEMS];
#pragma unroll
    for (int t = 0; t < FM_SELECT_ITEMS; ++t) {
        const int64_t j = j0 + (int64_t)t * FM_SELECT_BLOCK;
        k[t] = j < m ? select_index(index[j], n) : -1;
        alive[t] = k[t] >= 0;
        k[t] = k[t] < 0 ? 0 : k[t] > n - 1 ? n - 1 : k[t];                           // the clamp before every load below
    }
#pragma unroll
    for (int v = 0; v < FM_SELECT_MAX_VALUES; ++v) {
        if ((uint32_t)v < A.n_values) {
            const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(A.values[v]);
            uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.values_out[v]);
            uint32_t x[FM_SELECT_ITEMS];
#pragma unroll
            for (int t = 0; t < FM_SELECT_ITEMS; ++t) x[t] = src[k[t]];               // (a dead lane reads a valid element and drops it)
#pragma unroll
            for (int t = 0; t < FM_SELECT_ITEMS; ++t) {
                const int64_t j = j0 + (int64_t)t * FM_SELECT_BLOCK;
                if (j < m) out[j] = alive[t] ? x[t] : FM_SELECT_NAN_BITS;
            }
        }
    }
}

hipError_t launch_select_count(const DevCompressArgs& a, hipStream_t st)
{
    if (!select_count_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t blocks = prefix_blocks((int64_t)a.n);
    hipLaunchKernelGGL(fm_select_count_kernel, dim3(blocks), dim3(FM_PREFIX_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_select_carry_kernel, dim3(1), dim3(FM_PREFIX_CARRY_BLOCK), 0, st, a, blocks);
    return hipGetLastError();
}

hipError_t launch_select_compress(const DevCompressArgs& a, hipStream_t st)
{
    if (!select_shape_ok(a, false)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_select_compress_kernel, dim3(prefix_blocks((int64_t)a.n)), dim3(FM_PREFIX_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_select_expand(const DevCompressArgs& a, hipStream_t st)
{
    if (!select_shape_ok(a, true)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_select_expand_kernel, dim3(prefix_blocks((int64_t)a.n)), dim3(FM_PREFIX_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_select_gather(const DevIndexGatherArgs& a, hipStream_t st)
{
    if (!gather_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t grid = (uint32_t)(((int64_t)a.m + FM_SELECT_TILE - 1) / FM_SELECT_TILE);
    hipLaunchKernelGGL(fm_select_gather_kernel, dim3(grid), dim3(FM_SELECT_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
