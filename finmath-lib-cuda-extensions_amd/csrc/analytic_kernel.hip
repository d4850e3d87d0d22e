// analytic_kernel.hip — fm_function_apply_kernel and fm_option_formula_kernel for gfx950 (MI355X, CDNA4): the normal distribution function,
// its density and its quantile at every element of a vector, and the Black–Scholes and Bachelier formulas per path.  DESIGN.md §4.21;
// contract: include/fmhip.h; definition: host/normal_functions.hpp (every function evaluated here is ITS function, compiled for the device:
// + − × /, sqrt, comparisons and integer operations in fp64, no contraction — the bits are the host's); engine side: analytic_engine.hpp.
//
// The frame is table_kernel.hip's: 16-byte loads and stores, 256 lanes, a grid-stride loop over groups of four elements with a capped grid,
// a lane's NEXT group loaded before the current one is evaluated.  A vector's storage is a multiple of 256 bytes (Pool::alloc rounds the
// capacity), so the last group is read and written whole: what lies past n is inside the buffer, and every bit pattern is an argument
// these functions take.  No LDS.  The coefficients of Φ are constants of the code object, read by a piece index that differs between
// lanes: loads from constant memory, no register array is indexed at run time, no scratch.
// Per element of fm_function_apply_kernel the density is computed ONCE for Φ and φ (Φ = φ · Mills ratio), each distinct function once, and a
// repeated kind is a copy.  Which functions and outputs a launch wants is uniform: those branches are scalar.  The rare sides — the
// quantile's tails, Φ beyond |x| = 8, a degenerate formula element — are branches of the definition, marked unlikely where they are taken
// per element.
// The kernels trust their arguments: the launchers refuse what function_shape_ok / formula_shape_ok refuse.
#include <hip/hip_runtime.h>

#include "analytic_kernel.h"

namespace fm {

typedef float an_f32x4 __attribute__((ext_vector_type(4)));
typedef an_f32x4 __attribute__((address_space(1))) an_gfloat4;

template <int T>
__global__ void __launch_bounds__(FM_ANALYTIC_BLOCK) fm_function_apply_kernel(const DevFunctionArgs A)
{
    using namespace fmhost;
    bool want_cdf = false, want_density = false, want_quantile = false;
#pragma unroll
    for (int f = 0; f < T; ++f) {
        want_cdf |= A.kinds[f] == (uint32_t)FM_FN_NORMAL_CDF;
        want_density |= A.kinds[f] == (uint32_t)FM_FN_NORMAL_DENSITY;
        want_quantile |= A.kinds[f] == (uint32_t)FM_FN_NORMAL_QUANTILE;
    }
    const int64_t n = A.n;
    const an_gfloat4* __restrict__ px = reinterpret_cast<const an_gfloat4*>(A.x);
    const int64_t stride = (int64_t)gridDim.x * FM_ANALYTIC_BLOCK;
    int64_t i4 = (int64_t)blockIdx.x * FM_ANALYTIC_BLOCK + threadIdx.x;
    an_f32x4 ahead = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (i4 * 4 < n) ahead = px[i4];
#pragma unroll 1
    for (; i4 * 4 < n; i4 += stride) {
        const an_f32x4 xv = ahead;
        if ((i4 + stride) * 4 < n) ahead = px[i4 + stride];          // the next group is on its way while this one is evaluated
        an_f32x4 r[T];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double X = (double)xv[j];
            float cdf = 0.0f, density = 0.0f, quantile = 0.0f;
            if (want_cdf || want_density) {
                const double d = fm_normal_density(X);
                density = fm_narrow(d);
                if (want_cdf) cdf = fm_narrow(fm_normal_cdf_with(X, d));
            }
            if (want_quantile) quantile = fm_narrow(fm_normal_quantile_checked(X));
#pragma unroll
            for (int f = 0; f < T; ++f)
                r[f][j] = A.kinds[f] == (uint32_t)FM_FN_NORMAL_CDF ? cdf : A.kinds[f] == (uint32_t)FM_FN_NORMAL_DENSITY ? density : quantile;
        }
#pragma unroll
        for (int f = 0; f < T; ++f) reinterpret_cast<an_gfloat4*>(A.out[f])[i4] = r[f];
    }
}

template <int MODEL>
__global__ void __launch_bounds__(FM_ANALYTIC_BLOCK) fm_option_formula_kernel(const DevFormulaArgs A)
{
    using namespace fmhost;
    const int64_t n = A.n;
    const an_gfloat4* __restrict__ p0 = reinterpret_cast<const an_gfloat4*>(A.in[0]);
    const an_gfloat4* __restrict__ p1 = reinterpret_cast<const an_gfloat4*>(A.in[1]);
    const an_gfloat4* __restrict__ p2 = reinterpret_cast<const an_gfloat4*>(A.in[2]);
    const bool v0 = A.in[0] != 0, v1 = A.in[1] != 0, v2 = A.in[2] != 0;
    const bool want_value = (A.outputs & FM_FORMULA_VALUE) != 0, want_delta = (A.outputs & FM_FORMULA_DELTA) != 0, want_vega = (A.outputs & FM_FORMULA_VEGA) != 0;
    const int slot_delta = want_value ? 1 : 0, slot_vega = slot_delta + (want_delta ? 1 : 0);
    an_gfloat4* __restrict__ o_value = reinterpret_cast<an_gfloat4*>(A.out[0]);
    an_gfloat4* __restrict__ o_delta = reinterpret_cast<an_gfloat4*>(slot_delta == 0 ? A.out[0] : A.out[1]);
    an_gfloat4* __restrict__ o_vega = reinterpret_cast<an_gfloat4*>(slot_vega == 0 ? A.out[0] : slot_vega == 1 ? A.out[1] : A.out[2]);
    const double root_T = A.root_T, K = A.strike;
    const int64_t stride = (int64_t)gridDim.x * FM_ANALYTIC_BLOCK;
    int64_t i4 = (int64_t)blockIdx.x * FM_ANALYTIC_BLOCK + threadIdx.x;
    const an_f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
    an_f32x4 a0 = zero, a1 = zero, a2 = zero;
    if (i4 * 4 < n) {
        if (v0) a0 = p0[i4];
        if (v1) a1 = p1[i4];
        if (v2) a2 = p2[i4];
    }
#pragma unroll 1
    for (; i4 * 4 < n; i4 += stride) {
        const an_f32x4 f4 = a0, s4 = a1, n4 = a2;
        if ((i4 + stride) * 4 < n) {                                 // the next groups are on their way while these are evaluated
            if (v0) a0 = p0[i4 + stride];
            if (v1) a1 = p1[i4 + stride];
            if (v2) a2 = p2[i4 + stride];
        }
        an_f32x4 r_value = zero, r_delta = zero, r_vega = zero;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const FmFormulaOut r = fm_option_formula(MODEL, v0 ? (double)f4[j] : A.scalar[0], v1 ? (double)s4[j] : A.scalar[1], v2 ? (double)n4[j] : A.scalar[2], root_T, K);
            r_value[j] = fm_narrow(r.value); r_delta[j] = fm_narrow(r.delta); r_vega[j] = fm_narrow(r.vega);
        }
        if (want_value) o_value[i4] = r_value;
        if (want_delta) o_delta[i4] = r_delta;
        if (want_vega) o_vega[i4] = r_vega;
    }
}

hipError_t launch_function_apply(const DevFunctionArgs& a, hipStream_t st)
{
    if (!function_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(analytic_blocks(a.n)), block(FM_ANALYTIC_BLOCK);
    switch (a.n_functions) {
    case 1: hipLaunchKernelGGL(fm_function_apply_kernel<1>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL(fm_function_apply_kernel<2>, grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL(fm_function_apply_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(fm_function_apply_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_option_formula(const DevFormulaArgs& a, hipStream_t st)
{
    if (!formula_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(analytic_blocks(a.n)), block(FM_ANALYTIC_BLOCK);
    if (a.model == (uint32_t)fmhost::FM_FORMULA_BLACK_SCHOLES) hipLaunchKernelGGL(fm_option_formula_kernel<fmhost::FM_FORMULA_BLACK_SCHOLES>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(fm_option_formula_kernel<fmhost::FM_FORMULA_BACHELIER>, grid, block, 0, st, a);
    return hipGetLastError();
}

} // namespace fm
