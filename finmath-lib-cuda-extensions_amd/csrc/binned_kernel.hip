// binned_kernel.hip — fm_binned_xmom_kernel and fm_binned_eval_kernel for gfx950 (MI355X, CDNA4): the normal equations of a LOCALIZED
// least-squares regression — one small block per bin of a key vector — in one pass, and the piecewise estimate as a new vector.
// DESIGN.md §4.13; contract: include/fmhip.h; definition: host/binned_regression.hpp; engine side: binned_engine.hpp.
//
// Bins.  The n_bins - 1 ascending bounds sit in LDS, padded with +inf to 63; bin(k) = #{ j : bounds[j] < (double)k } is found by a
// branch-free search of six levels (a lower bound by binary lifting, no branch on the data).  A NaN key belongs to no bin.
//
// Accumulation (shape (a) of the issue: lane-private accumulators).  Every lane owns a column of running fp64 sums in LDS,
// acc[entry][lane] with entry = (bin, product): consecutive lanes touch consecutive 8-byte words, so no access conflicts, nothing is shared
// between lanes, and there is no atomic of any kind on a float.  A product of two fp32 values is exact in fp64, so fma(a, b, acc) adds the
// exact product and rounds once.  72 entries x 256 lanes x 8 B = 144 KB of the CU's 160 KB: one workgroup per CU.  Where bins x products
// exceed 72 entries the BINS are cut into slices along blockIdx.y; a slice reads the vectors again (from L2 / MALL mostly) and adds only
// the elements of its own bins.
//
// Order of the additions of one (bin, product): a lane adds its elements tile by tile, element by element (an element of another bin, or past
// n, adds nothing — which equals adding +0.0: a running sum that starts at +0.0 is never -0.0); the 64 lanes of a wave by the plain butterfly
// (bit 5 of the lane first); the tail — the waves, the workgroups of a slice, the arrivals, the host's flag — is side_pass_device.hpp's.
// The grid along x is binned_blocks(n) and the element a lane holds is a function of n alone: the bits of a sum depend on
// n, on which positions fall into the bin and on the two vectors' values there — not on the other vectors, roles, positions in the lists,
// the slicing, or the bounds of other bins.
// The kernels trust their arguments: the launchers refuse what binned_*_shape_ok refuse.  No register array is indexed at run time: no scratch.
#include <hip/hip_runtime.h>

#include "binned_kernel.h"
#include "os_device.hpp"
#include "side_pass_device.hpp"

namespace fm {

typedef float bn_f32x4 __attribute__((ext_vector_type(4)));
typedef bn_f32x4 __attribute__((address_space(1))) bn_gfloat4;

// bounds below kd among the 63 padded ones: six levels, the last index read is 62
__device__ __forceinline__ uint32_t bn_bin_of(const double* b, const double kd)
{
    uint32_t pos = 0u;
#pragma unroll
    for (uint32_t half = 32u; half != 0u; half >>= 1) {
        const uint32_t t = pos + half;
        pos = b[t - 1u] < kd ? t : pos;
    }
    return pos;
}

__device__ __forceinline__ void bn_load_bounds(double* b, const double* __restrict__ bounds, const uint32_t n_bins)
{
    for (uint32_t i = threadIdx.x; i < 64u; i += blockDim.x) b[i] = i + 1u < n_bins ? bounds[i] : __longlong_as_double(0x7ff0000000000000ll);
}

__global__ void __launch_bounds__(FM_BINNED_BLOCK) fm_binned_xmom_kernel(const DevBinnedXmomArgs A)
{
    __shared__ double acc[FM_BINNED_ENTRIES * FM_BINNED_BLOCK];
    __shared__ double wave_part[FM_BINNED_BLOCK / 64][FM_BINNED_ENTRIES];
    __shared__ double b[64];
    __shared__ uint32_t cnt[FM_BINNED_MAX_BINS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slice = blockIdx.y;
    const uint32_t qe = A.entries_per_bin;
    const uint32_t b_lo = slice * A.bins_per_slice;
    const uint32_t nb = A.n_bins - b_lo < A.bins_per_slice ? A.n_bins - b_lo : A.bins_per_slice;
    const uint32_t used = nb * qe;                                  // <= FM_BINNED_ENTRIES (binned_xmom_shape_ok)
    bn_load_bounds(b, A.bounds, A.n_bins);
    if (tid < (uint32_t)FM_BINNED_MAX_BINS) cnt[tid] = 0u;
    for (uint32_t e = 0; e < used; ++e) acc[e * FM_BINNED_BLOCK + tid] = 0.0;
    __syncthreads();
    const int64_t n = A.n;
    const bn_f32x4 ones = { 1.0f, 1.0f, 1.0f, 1.0f };
    const bn_gfloat4* __restrict__ pk = reinterpret_cast<const bn_gfloat4*>(A.key);
    const bool counting = slice == 0u;
#pragma unroll 1
    for (uint32_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint32_t i4 = tile * FM_BINNED_BLOCK + tid;
        const uint32_t at = (int64_t)i4 * 4 < n ? i4 : 0u;          // a partially valid float4 is in bounds: vectors are padded to 256 B
        const bn_f32x4 kv = pk[at];
        bn_f32x4 xv[FM_BINNED_MAX_X], yv[FM_BINNED_MAX_Y];
#pragma unroll
        for (int i = 0; i < FM_BINNED_MAX_X; ++i) {
            const bn_gfloat4* __restrict__ p = reinterpret_cast<const bn_gfloat4*>(A.x[i]);
            xv[i] = ((uint32_t)i < A.n_x && p) ? p[at] : ones;
        }
#pragma unroll
        for (int m = 0; m < FM_BINNED_MAX_Y; ++m) {
            const bn_gfloat4* __restrict__ p = reinterpret_cast<const bn_gfloat4*>(A.y[m]);
            yv[m] = (uint32_t)m < A.n_y ? p[at] : ones;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float k = kv[j];
            const bool valid = (int64_t)i4 * 4 + j < n && k == k;
            const uint32_t bin = bn_bin_of(b, (double)k);
            if (counting) os_lds_add(cnt, bin, valid);                  // integers: the order does not matter
            const uint32_t local = bin - b_lo;
            if (valid && local < nb) {
                double* a = acc + (size_t)(local * qe) * FM_BINNED_BLOCK + tid;
                double xd[FM_BINNED_MAX_X], yd[FM_BINNED_MAX_Y];
#pragma unroll
                for (int i = 0; i < FM_BINNED_MAX_X; ++i) xd[i] = (double)xv[i][j];
#pragma unroll
                for (int m = 0; m < FM_BINNED_MAX_Y; ++m) yd[m] = (double)yv[m][j];
                int s = 0;
#pragma unroll
                for (int i = 0; i < FM_BINNED_MAX_X; ++i)
#pragma unroll
                    for (int c = i; c < FM_BINNED_MAX_X; ++c, ++s) {
                        const int e = A.slot_entry[s];
                        if (e >= 0) a[e * FM_BINNED_BLOCK] = __builtin_fma(xd[i], xd[c], a[e * FM_BINNED_BLOCK]);      // the product is exact: one rounding
                    }
#pragma unroll
                for (int i = 0; i < FM_BINNED_MAX_X; ++i)
#pragma unroll
                    for (int m = 0; m < FM_BINNED_MAX_Y; ++m, ++s) {
                        const int e = A.slot_entry[s];
                        if (e >= 0) a[e * FM_BINNED_BLOCK] = __builtin_fma(xd[i], yd[m], a[e * FM_BINNED_BLOCK]);
                    }
            }
        }
    }
    __syncthreads();
    if (counting && tid < A.n_bins) {
        const uint32_t c = cnt[tid];
        if (c) __hip_atomic_fetch_add(A.counts_dev + tid, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t e = 0; e < used; ++e) {
        const double v = pass_wave_sum(acc[e * FM_BINNED_BLOCK + tid]);
        if (lane == 0u) wave_part[wave][e] = v;
    }
    __syncthreads();
    // the counts go to pinned memory with the sums of slice 0; the device array is zero again behind them
    const auto publish_counts = [&] {
        if (counting && tid < A.n_bins) {
            A.counts_host[tid] = __hip_atomic_load(A.counts_dev + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(A.counts_dev + tid, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    pass_combine_partials<FM_BINNED_BLOCK>(&wave_part[0][0], FM_BINNED_ENTRIES, used, A.partials + (size_t)slice * FM_BINNED_ENTRIES * gridDim.x,
                                           A.out_host + (size_t)b_lo * qe, A.counters + slice, A.counters + FM_BINNED_MAX_SLICES, A.done_flag, A.done_value,
                                           publish_counts);
}

// out[p] = ((x_0[p]·c_0) + x_1[p]·c_1) + x_2[p]·c_2 with the coefficients of bin(key[p]): fp32 products and sums that round one by one
// (__fmul_rn / __fadd_rn are never contracted).  Bounds and the narrowed coefficients in LDS; a NaN key gives NaN.
__global__ void __launch_bounds__(FM_BINNED_BLOCK) fm_binned_eval_kernel(const DevBinnedEvalArgs A)
{
    __shared__ double b[64];
    __shared__ float coef[FM_BINNED_MAX_BINS * FM_BINNED_MAX_X];
    bn_load_bounds(b, A.bounds, A.n_bins);
    for (uint32_t i = threadIdx.x; i < A.n_bins * A.n_x; i += FM_BINNED_BLOCK) coef[i] = A.coefficients[i];
    __syncthreads();
    const int64_t n = A.n;
    const uint32_t nx = A.n_x;
    const bn_f32x4 ones = { 1.0f, 1.0f, 1.0f, 1.0f };
    const bn_gfloat4* __restrict__ pk = reinterpret_cast<const bn_gfloat4*>(A.key);
    const bn_gfloat4* __restrict__ p0 = reinterpret_cast<const bn_gfloat4*>(A.x[0]);
    const bn_gfloat4* __restrict__ p1 = reinterpret_cast<const bn_gfloat4*>(A.x[1]);
    const bn_gfloat4* __restrict__ p2 = reinterpret_cast<const bn_gfloat4*>(A.x[2]);
    bn_gfloat4* __restrict__ po = reinterpret_cast<bn_gfloat4*>(A.out);
#pragma unroll 1
    for (int64_t i4 = (int64_t)blockIdx.x * FM_BINNED_BLOCK + threadIdx.x; i4 * 4 < n; i4 += (int64_t)gridDim.x * FM_BINNED_BLOCK) {
        const bn_f32x4 kv = pk[i4];
        const bn_f32x4 x0 = p0 ? p0[i4] : ones;
        const bn_f32x4 x1 = (nx > 1u && p1) ? p1[i4] : ones;
        const bn_f32x4 x2 = (nx > 2u && p2) ? p2[i4] : ones;
        bn_f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float k = kv[j];
            const uint32_t at = bn_bin_of(b, (double)k) * nx;
            float v = __fmul_rn(x0[j], coef[at]);
            if (nx > 1u) v = __fadd_rn(v, __fmul_rn(x1[j], coef[at + 1u]));
            if (nx > 2u) v = __fadd_rn(v, __fmul_rn(x2[j], coef[at + 2u]));
            r[j] = k == k ? v : __uint_as_float(0x7fc00000u);
        }
        po[i4] = r;
    }
}

hipError_t launch_binned_xmom(const DevBinnedXmomArgs& a, hipStream_t st)
{
    if (!binned_xmom_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_binned_xmom_kernel, dim3(binned_blocks(a.n), a.n_slices, 1), dim3(FM_BINNED_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_binned_eval(const DevBinnedEvalArgs& a, hipStream_t st)
{
    if (!binned_eval_shape_ok(a)) return hipErrorInvalidValue;
    int64_t blocks = (a.n + FM_BINNED_TILE - 1) / FM_BINNED_TILE;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(fm_binned_eval_kernel, dim3((uint32_t)blocks), dim3(FM_BINNED_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
