// nested_kernel.hip — fm_block_moments_kernel, fm_block_combine_kernel and fm_repeat_kernel for gfx950 (MI355X, CDNA4): the two operations
// that change the SHAPE of a sample on the device — k inner paths per outer state (repeat), and the inner payoffs averaged per outer path
// (block moments).  DESIGN.md §4.22; contract: include/fmhip.h; definition: host/block_moments.hpp, whose order of additions every sum
// below restates (-ffp-contract=off, no fast math: every fl(a + b) is one rounded fp64 addition); launchers: nested_kernel.h; engine side:
// nested_engine.hpp.
//
// The unit of work is a WAVE's task; a workgroup is four waves that share nothing (no LDS, no barrier), blockIdx.y is the vector's slot in
// the call, and the waves of the grid stride over the tasks.  Which regime runs is a function of `block` alone:
//   small   block <= 64: w = the power of two >= block lanes per block, 64 / w blocks per task.  Lane (g, i) loads element i of the task's
//           block g — the wave's loads are one contiguous run across the blocks' boundaries, whatever their alignment — and the butterfly
//           stops at w: the rounds off = w/2 … 1 stay inside the block's lanes (the segmented reduction).  Lanes i >= block hold −0.0.
//   medium  64 < block <= 2048: one task per block.  Lane l walks the elements l, l + 64, … of the block (every load instruction of the wave
//           is 256 contiguous bytes), then the butterfly over the 64 lanes (pass_wave_sum: bit 5 first — the order of the definition).
//   large   block > 2048: one task per SEGMENT of 2048 elements, reduced as a medium block, its { s1, s2 } stored to the side-pass scratch
//           with plain stores; fm_block_combine_kernel, chained behind on the stream, reduces a block's segment sums the same way — lane l
//           walks the partials l, l + 64, … — and writes the outputs.  No workgroup waits for another; no atomics at all.
// A lane's walk starts from −0.0: fl(−0.0 + x) = x bit for bit for every x that is no NaN, so "the first term taken as it is" and "a leaf
// without a term is −0.0" of the definition are both this.  Loads are 4 bytes per lane: a block starts at any element, so nothing wider is
// aligned in general, and the walk — which IS the definition — is per element.  Every address is below n (int64 arithmetic; n <= 2^31 − 1).
//
// fm_repeat_kernel: out[(t·n + p)·each + e] = v[p], copied as 32-bit patterns.  A lane owns four consecutive OUTPUT elements and stores
// them with one 16-byte store (storage is 256-byte aligned and padded: the last quad is inside it); its source elements are read through
// the vector cache — neighbouring lanes of a wave read the same or adjacent words, one load instruction per output quad.
#include <hip/hip_runtime.h>

#include "nested_kernel.h"
#include "side_pass_device.hpp"

namespace fm {

typedef uint32_t nk_u32x4 __attribute__((ext_vector_type(4)));
typedef double nk_f64x2 __attribute__((ext_vector_type(2)));

// the outputs of block q of vector `slot` from its sums, by one lane
__device__ __forceinline__ void nk_write(const DevBlockMomentsArgs& A, const uint32_t slot, const int64_t q, const double s1, const double s2)
{
    fmhost::BlockSums s; s.s1 = s1; s.s2 = s2;
    int j = 0;
#pragma unroll
    for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1)
        if (A.mask & (uint32_t)bit) reinterpret_cast<float*>(A.out[slot][j++])[q] = fmhost::fm_block_output(bit, s, A.block);
}

__global__ void __launch_bounds__(FM_NESTED_BLOCK) fm_block_moments_kernel(const DevBlockMomentsArgs A)
{
    const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.y;
    const int64_t wave0 = (int64_t)blockIdx.x * FM_NESTED_WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * FM_NESTED_WAVES;
    const float* __restrict__ v = reinterpret_cast<const float*>(A.v[slot]);
    const int64_t block = A.block, m = A.n / block;
    if (block <= FM_NESTED_SMALL) {
        const uint32_t w = (uint32_t)fmhost::fm_block_width(block), per = 64u / w, g = lane / w, i = lane & (w - 1u);
        const int64_t tasks = (m + per - 1) / per;
#pragma unroll 1
        for (int64_t task = wave0; task < tasks; task += waves) {
            const int64_t q = task * per + g;
            const bool mine = q < m && (int64_t)i < block;
            double x = -0.0, y = -0.0;
            if (mine) { x = (double)v[q * block + i]; y = x * x; }
#pragma unroll
            for (uint32_t off = 32u; off > 0u; off >>= 1) {
                if (off < w) { x = x + __shfl_xor(x, (int)off, 64); y = y + __shfl_xor(y, (int)off, 64); }      // (w is the wave's: a scalar branch)
            }
            if (mine && i == 0u) nk_write(A, slot, q, x, y);
        }
        return;
    }
    const int64_t segments = fmhost::fm_block_segments(block), tasks = m * segments;
#pragma unroll 1
    for (int64_t task = wave0; task < tasks; task += waves) {
        const int64_t q = task / segments, s = task - q * segments;
        const int64_t e0 = s * fmhost::FM_BLOCK_SEGMENT;
        const int64_t count = block - e0 < fmhost::FM_BLOCK_SEGMENT ? block - e0 : fmhost::FM_BLOCK_SEGMENT;
        const float* __restrict__ p = v + q * block + e0 + lane;
        double x = -0.0, y = -0.0;
        if (count == fmhost::FM_BLOCK_SEGMENT) {
#pragma unroll 8
            for (int k = 0; k < (int)(fmhost::FM_BLOCK_SEGMENT / 64); ++k) { const double t = (double)p[k * 64]; x = x + t; y = y + t * t; }
        } else {
            const int64_t mine = count - (int64_t)lane;                               // the lane has elements k·64 < mine
#pragma unroll 4
            for (int64_t k = 0; k < count; k += 64) {                                 // (a uniform trip count: the loads of four rounds are in flight together)
                const bool has = k < mine;
                const double t = has ? (double)p[k] : -0.0;
                x = x + t; y = y + (has ? t * t : -0.0);
            }
        }
        x = pass_wave_sum(x);
        y = pass_wave_sum(y);
        if (lane == 0u) {
            if (segments == 1) nk_write(A, slot, q, x, y);
            else {
                nk_f64x2 both; both[0] = x; both[1] = y;
                reinterpret_cast<nk_f64x2*>(A.partials)[((int64_t)slot * m + q) * segments + s] = both;
            }
        }
    }
}

// large blocks, second stage: one task per block over its `segments` partials
__global__ void __launch_bounds__(FM_NESTED_BLOCK) fm_block_combine_kernel(const DevBlockMomentsArgs A)
{
    const uint32_t lane = threadIdx.x & 63u, slot = blockIdx.y;
    const int64_t wave0 = (int64_t)blockIdx.x * FM_NESTED_WAVES + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * FM_NESTED_WAVES;
    const int64_t m = A.n / A.block, segments = fmhost::fm_block_segments(A.block);
#pragma unroll 1
    for (int64_t q = wave0; q < m; q += waves) {
        const nk_f64x2* __restrict__ p = reinterpret_cast<const nk_f64x2*>(A.partials) + ((int64_t)slot * m + q) * segments;
        double x = -0.0, y = -0.0;
#pragma unroll 4
        for (int64_t k = lane; k < segments; k += 64) { const nk_f64x2 t = p[k]; x = x + t[0]; y = y + t[1]; }
        x = pass_wave_sum(x);
        y = pass_wave_sum(y);
        if (lane == 0u) nk_write(A, slot, q, x, y);
    }
}

__global__ void __launch_bounds__(FM_NESTED_BLOCK) fm_repeat_kernel(const DevRepeatArgs A)
{
    const uint32_t n = (uint32_t)A.n, each = (uint32_t)A.each;
    const uint32_t total = (uint32_t)(A.n * A.each * A.times), quads = (total + 3u) / 4u;      // <= 2^31 − 1: checked by the launcher
    const uint32_t* __restrict__ v = reinterpret_cast<const uint32_t*>(A.v);
    nk_u32x4* __restrict__ out = reinterpret_cast<nk_u32x4*>(A.out);
    const uint32_t stride = gridDim.x * (uint32_t)FM_NESTED_BLOCK;                             // <= 2^20
#pragma unroll 1
    for (uint64_t g = (uint64_t)blockIdx.x * FM_NESTED_BLOCK + threadIdx.x; g < (uint64_t)quads; g += stride) {
        const uint32_t o = (uint32_t)g * 4u;
        const uint32_t pe = o / each;                  // (t·n + p)
        uint32_t e = o - pe * each, p = pe % n;
        nk_u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = v[p];                               // (p < n always: past `total` the quad's tail lies in the padding and repeats the walk)
            if (++e == each) { e = 0u; if (++p == n) p = 0u; }
        }
        out[g] = r;
    }
}

hipError_t launch_block_moments(const DevBlockMomentsArgs& a, hipStream_t st)
{
    if (!block_moments_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_block_moments_kernel, dim3(nested_grid(block_tasks(a.n, a.block)), a.n_vectors), dim3(FM_NESTED_BLOCK), 0, st, a);
    if (block_is_large(a.block))
        hipLaunchKernelGGL(fm_block_combine_kernel, dim3(nested_grid(a.n / a.block), a.n_vectors), dim3(FM_NESTED_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_repeat(const DevRepeatArgs& a, hipStream_t st)
{
    if (!repeat_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t quads = (a.n * a.each * a.times + 3) / 4, blocks = (quads + FM_NESTED_BLOCK - 1) / FM_NESTED_BLOCK;
    hipLaunchKernelGGL(fm_repeat_kernel, dim3((uint32_t)(blocks > FM_NESTED_MAX_BLOCKS ? FM_NESTED_MAX_BLOCKS : blocks)), dim3(FM_NESTED_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
