// kreg_kernel.hip — fm_kernel_moments_kernel for gfx950 (MI355X, CDNA4): the kernel-weighted local moments of up to 4 vectors at up to 256
// points of a key vector in one pass — E[y | x = p_q] as a curve, the inner step of the particle method for local-stochastic volatility.
// DESIGN.md §4.19; contract: include/fmhip.h; definition: host/kernel_regression.hpp (the weight and the terms are ITS functions, compiled
// here for the device); engine side: kreg_engine.hpp.  A close relative of fm_binned_xmom_kernel (binned_kernel.hip) with soft, overlapping
// bins: the accumulator layout is that kernel's, and the tail is side_pass_device.hpp's.
//
// Points.  lower, upper (padded with +inf to the power of two above Q), points and rh sit in LDS.  The members of xd = (double)key[i] are the
// points q ∈ [a, b), a = #{ q : upper_q <= xd }, b = #{ q : lower_q < xd }: two branch-free lower bounds by binary lifting, clamped to Q.  A NaN
// finds a = b = 0, −inf too, +inf a = b = Q.  The loop over the members of an element is the one data-dependent loop: it runs over
// [max(a, slice_lo), min(b, slice_hi)), and slice_hi <= Q comes from the arguments; no address depends on the key but through a and b.
//
// Accumulation.  Every lane owns a column of running fp64 sums in LDS, acc[entry][lane] with entry = (point of the slice, term): consecutive
// lanes touch consecutive 8-byte words, nothing is shared between lanes, no atomic on a float.  A term is rounded once where it is formed
// and added with a plain fp64 addition (the build has -ffp-contract=off).  72 entries x 256 lanes x 8 B = 144 KB, the four tables 12 KB, of
// the CU's 160 KB: one workgroup per CU.  Where Q x entries_per_point exceeds 72 the POINTS are cut into slices along blockIdx.y; a slice
// reads the vectors again and adds only the members of its own points.
//
// Order of the additions of one (point, term): a lane adds its elements tile by tile, element by element (a non-member adds nothing — which
// equals adding +0.0: a running sum that starts at +0.0 is never −0.0); the 64 lanes of a wave by the plain butterfly
// (bit 5 of the lane first); the waves and the workgroups of a slice as pass_combine_partials adds them.  The grid along x is
// binned_blocks(n): the bits of a sum depend on n, on which positions are members and on the values
// there — not on the other points, the slicing, n_y, or the slot of a vector.
// The kernel trusts its arguments: the launcher refuses what kernel_moments_shape_ok refuses.  No register array is indexed at run time: no scratch.
#include <hip/hip_runtime.h>

#include "kreg_kernel.h"
#include "side_pass_device.hpp"
#include "../host/kernel_regression.hpp"

namespace fm {

typedef float kr_f32x4 __attribute__((ext_vector_type(4)));
typedef kr_f32x4 __attribute__((address_space(1))) kr_gfloat4;

// #{ j : t[j] < xd } (STRICT) or #{ j : t[j] <= xd } among the 2·half − 1 padded entries: the last index read is 2·half − 2
template <bool STRICT>
__device__ __forceinline__ uint32_t kr_count_below(const double* t, const uint32_t half0, const double xd)
{
    uint32_t pos = 0u;
#pragma unroll 1
    for (uint32_t half = half0; half != 0u; half >>= 1) {
        const uint32_t at = pos + half;
        const double v = t[at - 1u];
        pos = (STRICT ? v < xd : v <= xd) ? at : pos;
    }
    return pos;
}

__global__ void __launch_bounds__(FM_KREG_BLOCK) fm_kernel_moments_kernel(const DevKernelMomentsArgs A)
{
    __shared__ double acc[FM_KREG_ENTRIES * FM_KREG_BLOCK];
    __shared__ double wave_part[FM_KREG_BLOCK / 64][FM_KREG_ENTRIES];
    __shared__ double lower[FM_KREG_PAD], upper[FM_KREG_PAD];
    __shared__ double pts[FM_KREG_MAX_POINTS], rhs[FM_KREG_MAX_POINTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slice = blockIdx.y;
    const uint32_t Q = A.n_points, qe = A.entries_per_point, ny = A.n_y;
    const uint32_t s_lo = slice * A.points_per_slice;
    const uint32_t np = Q - s_lo < A.points_per_slice ? Q - s_lo : A.points_per_slice;
    const uint32_t s_hi = s_lo + np;                                // <= Q
    const uint32_t used = np * qe;                                  // <= FM_KREG_ENTRIES (kernel_moments_shape_ok)
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (uint32_t i = tid; i < (uint32_t)FM_KREG_PAD; i += FM_KREG_BLOCK) {
        lower[i] = i < Q ? A.tables[i] : inf;
        upper[i] = i < Q ? A.tables[Q + i] : inf;
    }
    for (uint32_t i = tid; i < (uint32_t)FM_KREG_MAX_POINTS; i += FM_KREG_BLOCK) {
        pts[i] = i < Q ? A.tables[2u * Q + i] : 0.0;
        rhs[i] = i < Q ? A.tables[3u * Q + i] : 0.0;
    }
    for (uint32_t e = 0; e < used; ++e) acc[e * FM_KREG_BLOCK + tid] = 0.0;
    __syncthreads();
    const int64_t n = A.n;
    const int kernel = (int)A.kernel;
    const bool linear = A.order != 0u;
    const uint32_t half0 = A.search_half;
    const kr_f32x4 zeros = { 0.0f, 0.0f, 0.0f, 0.0f };
    const kr_gfloat4* __restrict__ pk = reinterpret_cast<const kr_gfloat4*>(A.key);
#pragma unroll 1
    for (uint32_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint32_t i4 = tile * FM_KREG_BLOCK + tid;
        const uint32_t at = (int64_t)i4 * 4 < n ? i4 : 0u;          // a partially valid float4 is in bounds: vectors are padded to 256 B
        const kr_f32x4 kv = pk[at];
        kr_f32x4 yv[FM_KREG_MAX_Y];
#pragma unroll
        for (int m = 0; m < FM_KREG_MAX_Y; ++m) {
            const kr_gfloat4* __restrict__ p = reinterpret_cast<const kr_gfloat4*>(A.y[m]);
            yv[m] = (uint32_t)m < ny ? p[at] : zeros;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = (int64_t)i4 * 4 + j < n;
            const double xd = (double)kv[j];
            uint32_t a = kr_count_below<false>(upper, half0, xd);
            uint32_t b = kr_count_below<true>(lower, half0, xd);
            a = a < Q ? a : Q;
            b = b < Q ? b : Q;
            const uint32_t q_lo = a > s_lo ? a : s_lo;
            const uint32_t q_hi = valid ? (b < s_hi ? b : s_hi) : 0u;
            const double y0 = (double)yv[0][j], y1 = (double)yv[1][j], y2 = (double)yv[2][j], y3 = (double)yv[3][j];
#pragma unroll 1
            for (uint32_t q = q_lo; q < q_hi; ++q) {                // q_hi <= s_hi <= Q: bounded by the arguments
                const double d = xd - pts[q];
                const double w = fmhost::fm_kernel_weight(kernel, d, rhs[q]);
                double* c = acc + (size_t)((q - s_lo) * qe) * FM_KREG_BLOCK + tid;
                c[0] = c[0] + w;
                if (!linear) {
                    if (ny > 0u) c[1 * FM_KREG_BLOCK] = c[1 * FM_KREG_BLOCK] + w * y0;
                    if (ny > 1u) c[2 * FM_KREG_BLOCK] = c[2 * FM_KREG_BLOCK] + w * y1;
                    if (ny > 2u) c[3 * FM_KREG_BLOCK] = c[3 * FM_KREG_BLOCK] + w * y2;
                    if (ny > 3u) c[4 * FM_KREG_BLOCK] = c[4 * FM_KREG_BLOCK] + w * y3;
                }
                else {
                    const double e1 = w * d;
                    c[1 * FM_KREG_BLOCK] = c[1 * FM_KREG_BLOCK] + e1;
                    c[2 * FM_KREG_BLOCK] = c[2 * FM_KREG_BLOCK] + e1 * d;
                    double* cw = c + 3 * FM_KREG_BLOCK;
                    double* ce = cw + ny * FM_KREG_BLOCK;
                    if (ny > 0u) { cw[0 * FM_KREG_BLOCK] = cw[0 * FM_KREG_BLOCK] + w * y0; ce[0 * FM_KREG_BLOCK] = ce[0 * FM_KREG_BLOCK] + e1 * y0; }
                    if (ny > 1u) { cw[1 * FM_KREG_BLOCK] = cw[1 * FM_KREG_BLOCK] + w * y1; ce[1 * FM_KREG_BLOCK] = ce[1 * FM_KREG_BLOCK] + e1 * y1; }
                    if (ny > 2u) { cw[2 * FM_KREG_BLOCK] = cw[2 * FM_KREG_BLOCK] + w * y2; ce[2 * FM_KREG_BLOCK] = ce[2 * FM_KREG_BLOCK] + e1 * y2; }
                    if (ny > 3u) { cw[3 * FM_KREG_BLOCK] = cw[3 * FM_KREG_BLOCK] + w * y3; ce[3 * FM_KREG_BLOCK] = ce[3 * FM_KREG_BLOCK] + e1 * y3; }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t e = 0; e < used; ++e) {
        const double v = pass_wave_sum(acc[e * FM_KREG_BLOCK + tid]);
        if (lane == 0u) wave_part[wave][e] = v;
    }
    __syncthreads();
    pass_combine_partials<FM_KREG_BLOCK>(&wave_part[0][0], FM_KREG_ENTRIES, used, A.partials + (size_t)slice * FM_KREG_ENTRIES * gridDim.x,
                                         A.out_host + (size_t)s_lo * qe, A.counters + slice, A.counters + FM_KREG_MAX_SLICES, A.done_flag, A.done_value);
}

hipError_t launch_kernel_moments(const DevKernelMomentsArgs& a, hipStream_t st)
{
    if (!kernel_moments_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_kernel_moments_kernel, dim3(binned_blocks(a.n), a.n_slices, 1), dim3(FM_KREG_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
