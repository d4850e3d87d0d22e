// block_order_kernel.hip — fm_block_order_small_kernel and fm_block_order_medium_kernel<P> for gfx950 (MI355X, CDNA4): every block of a
// vector sorted by the 32-bit key of host/block_order.hpp in a bitonic network, and from the sorted keys the selected ranks, the range
// means or the sorted block itself.  DESIGN.md §4.23; contract: include/fmhip.h; definition: host/block_order.hpp, whose order of
// additions the range sums restate (-ffp-contract=off, no fast math); launcher: block_order_kernel.h; engine side: block_order_engine.hpp.
//
// One launch per call, blockIdx.y is the vector's slot, every input element is loaded once (4 bytes per lane, contiguous across the lanes:
// a block starts at any element).  No atomics, no workgroup waits for another, no scratch; every register array is indexed by unrolled,
// compile-time indices.  Which regime runs is a function of `block` alone:
//   small   block <= 64: w = the power of two >= block lanes per block, 64 / w blocks per wave task (the layout of fm_block_moments_kernel),
//           the waves of the grid stride over the tasks.  One key per lane; the network's compare-exchanges are __shfl_xor rounds, (k, j) with
//           j < k <= w.  No LDS.  Lanes i >= block hold 0xffffffff: they sort with the NaNs behind every rank < block.
//   medium  64 < block <= 4096: one workgroup of T = order_lanes(P) lanes per block (128 at P = 128, 256 up to P = 1024, 1024 above: the
//           grid's cap leaves one or two such workgroups per CU, and sixteen waves hide a round's latency where four do not), P = the power
//           of two >= block keys, element e = t + T·r in register r of lane t.  A stride j < 64 is a __shfl_xor round, a stride j >= T
//           exchanges two registers of one lane, and the strides 64 <= j < T between go through LDS (P keys, at most 16 KiB, a barrier
//           behind the writes and one behind the reads).  The workgroups of the grid stride over the blocks.
// The network sorts ascending: at (k, j) element e keeps the smaller key iff ((e & j) == 0) == ((e & k) == 0); at k = P, e & k == 0.
//
// Range sums come from the SORTED keys, as the definition makes them from an array of count = to − from + 1 elements: lane l walks the
// terms l, l + 64, … of a segment of 2048 in fp64 from −0.0, pass_wave_sum joins the 64 leaves (bit 5 first; leaves without a term hold
// −0.0, which is what the narrower butterfly of a short array is), and the second segment's sum is added to the first's (fm_block_unit of
// two terms).  In the small regime term l reaches lane l of its block by one __shfl, and the butterfly stops at w.
#include <hip/hip_runtime.h>

#include "block_order_kernel.h"
#include "side_pass_device.hpp"

namespace fm {

__device__ __forceinline__ uint32_t bo_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t bo_max(uint32_t a, uint32_t b) { return a < b ? b : a; }

__global__ void __launch_bounds__(FM_ORDER_SMALL_BLOCK) fm_block_order_small_kernel(const DevBlockOrderArgs A)
{
    const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.y;
    const int64_t wave0 = (int64_t)blockIdx.x * FM_ORDER_SMALL_WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * FM_ORDER_SMALL_WAVES;
    const uint32_t* __restrict__ v = reinterpret_cast<const uint32_t*>(A.v[slot]);
    const uint32_t block = (uint32_t)A.block;
    const int64_t m = A.n / A.block;
    const uint32_t w = (uint32_t)fmhost::fm_block_width(A.block), per = 64u / w, g = lane / w, i = lane & (w - 1u);
    const int64_t tasks = (m + per - 1) / per;
#pragma unroll 1
    for (int64_t task = wave0; task < tasks; task += waves) {
        const int64_t q = task * per + g;
        const bool mine = q < m && i < block;
        uint32_t key = fmhost::FM_ORDER_NAN_KEY;
        if (mine) key = fmhost::fm_order_key(v[q * block + i]);
#pragma unroll
        for (uint32_t k = 2u; k <= 64u; k <<= 1) {
            if (k <= w) {                                                                      // (w is the wave's: a scalar branch)
#pragma unroll
                for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
                    const uint32_t other = (uint32_t)__shfl_xor((int)key, (int)j, 64);
                    const bool smaller = ((i & j) == 0u) == ((i & k) == 0u);
                    key = smaller ? bo_min(key, other) : bo_max(key, other);
                }
            }
        }
        if (A.sort) {
            if (mine) reinterpret_cast<uint32_t*>(A.out[slot][0])[q * block + i] = fmhost::fm_order_bits(key);
            continue;
        }
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)fmhost::FM_BLOCK_ORDER_MAX_RANKS; ++j)
            if (j < A.n_ranks && mine && i == A.ranks[j]) reinterpret_cast<uint32_t*>(A.out[slot][j])[q] = fmhost::fm_order_bits(key);
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)fmhost::FM_BLOCK_ORDER_MAX_RANGES; ++j) {
            if (j < A.n_ranges) {                                                              // (uniform: every lane takes part in the shuffles)
                const uint32_t from = A.range_from[j], count = A.range_to[j] - from + 1u;
                const uint32_t term = (uint32_t)__shfl((int)key, (int)((lane - i) + ((from + i) & (w - 1u))), 64);      // sorted position from + i of this block
                double x = i < count ? fmhost::fm_order_term(term) : -0.0;
#pragma unroll
                for (uint32_t off = 32u; off > 0u; off >>= 1)
                    if (off < w) x = x + __shfl_xor(x, (int)off, 64);
                if (q < m && i == 0u) reinterpret_cast<float*>(A.out[slot][A.n_ranks + j])[q] = fmhost::fm_order_mean(x, (int64_t)count);
            }
        }
    }
}

template <int P>
__global__ void __launch_bounds__(order_lanes(P)) fm_block_order_medium_kernel(const DevBlockOrderArgs A)
{
    constexpr int T = order_lanes(P), R = P / T;
    __shared__ uint32_t lds[P];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, slot = blockIdx.y;
    const uint32_t* __restrict__ v = reinterpret_cast<const uint32_t*>(A.v[slot]);
    const uint32_t block = (uint32_t)A.block;
    const int64_t m = A.n / A.block;
#pragma unroll 1
    for (int64_t q = blockIdx.x; q < m; q += gridDim.x) {
        uint32_t key[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t e = t + (uint32_t)(T * r);
            key[r] = e < block ? fmhost::fm_order_key(v[q * block + e]) : fmhost::FM_ORDER_NAN_KEY;
        }
#pragma unroll
        for (int k = 2; k <= P; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (j >= T) {                                                                  // two registers of this lane
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if ((r & (j / T)) == 0) {
                            const int r2 = r | (j / T);
                            const bool ascending = (((int)t + T * r) & k) == 0;
                            const uint32_t lo = bo_min(key[r], key[r2]), hi = bo_max(key[r], key[r2]);
                            key[r] = ascending ? lo : hi;
                            key[r2] = ascending ? hi : lo;
                        }
                    }
                } else if (j >= 64) {                                                          // another wave's lane: through LDS
#pragma unroll
                    for (int r = 0; r < R; ++r) lds[t + (uint32_t)(T * r)] = key[r];
                    __syncthreads();
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t e = t + (uint32_t)(T * r), other = lds[e ^ (uint32_t)j];
                        const bool smaller = ((e & (uint32_t)j) == 0u) == ((e & (uint32_t)k) == 0u);
                        key[r] = smaller ? bo_min(key[r], other) : bo_max(key[r], other);
                    }
                    __syncthreads();
                } else {                                                                       // another lane of this wave
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t e = t + (uint32_t)(T * r), other = (uint32_t)__shfl_xor((int)key[r], j, 64);
                        const bool smaller = ((e & (uint32_t)j) == 0u) == ((e & (uint32_t)k) == 0u);
                        key[r] = smaller ? bo_min(key[r], other) : bo_max(key[r], other);
                    }
                }
            }
        }
        if (A.sort) {
            uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.out[slot][0]) + q * block;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t e = t + (uint32_t)(T * r);
                if (e < block) out[e] = fmhost::fm_order_bits(key[r]);
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) lds[t + (uint32_t)(T * r)] = key[r];
        __syncthreads();
        if (t < A.n_ranks) reinterpret_cast<uint32_t*>(A.out[slot][t])[q] = fmhost::fm_order_bits(lds[A.ranks[t]]);
#pragma unroll 1
        for (uint32_t j = wave; j < A.n_ranges; j += (uint32_t)(T / 64)) {                     // a wave per range
            const uint32_t from = A.range_from[j], count = A.range_to[j] - from + 1u;
            double S = -0.0;
#pragma unroll 1
            for (uint32_t s0 = 0u; s0 < count; s0 += (uint32_t)fmhost::FM_BLOCK_SEGMENT) {
                const uint32_t terms = count - s0 < (uint32_t)fmhost::FM_BLOCK_SEGMENT ? count - s0 : (uint32_t)fmhost::FM_BLOCK_SEGMENT;
                double x = -0.0;
#pragma unroll 4
                for (uint32_t l = lane; l < terms; l += 64u) x = x + fmhost::fm_order_term(lds[from + s0 + l]);
                x = pass_wave_sum(x);
                S = s0 == 0u ? x : S + x;
            }
            if (lane == 0u) reinterpret_cast<float*>(A.out[slot][A.n_ranks + j])[q] = fmhost::fm_order_mean(S, (int64_t)count);
        }
        __syncthreads();                                                                       // the next block's keys overwrite these
    }
}

template <int P>
static void bo_launch_medium(const DevBlockOrderArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(fm_block_order_medium_kernel<P>, dim3(order_grid(a.n, a.block), a.n_vectors), dim3(order_lanes(P)), 0, st, a);
}

hipError_t launch_block_order(const DevBlockOrderArgs& a, hipStream_t st)
{
    if (!block_order_shape_ok(a)) return hipErrorInvalidValue;
    if (order_is_small(a.block))
        hipLaunchKernelGGL(fm_block_order_small_kernel, dim3(order_grid(a.n, a.block), a.n_vectors), dim3(FM_ORDER_SMALL_BLOCK), 0, st, a);
    else switch (order_padded(a.block)) {
        case 128:  bo_launch_medium<128>(a, st); break;
        case 256:  bo_launch_medium<256>(a, st); break;
        case 512:  bo_launch_medium<512>(a, st); break;
        case 1024: bo_launch_medium<1024>(a, st); break;
        case 2048: bo_launch_medium<2048>(a, st); break;
        default:   bo_launch_medium<4096>(a, st); break;
    }
    return hipGetLastError();
}

} // namespace fm
