// implied_volatility_kernel.hip — fm_implied_volatility_kernel for gfx950 (MI355X, CDNA4): the implied volatility per path of a call price
// under the Black–Scholes or the Bachelier model, with ∂σ/∂price and ∂σ/∂forward at the root.  DESIGN.md §4.25; contract: include/fmhip.h;
// definition: host/implied_volatility.hpp (the function evaluated here is ITS function, compiled for the device: + − × /, sqrt, comparisons
// and integer operations in fp64, no contraction — the bits are the host's); engine side: implied_volatility_engine.hpp.
//
// The frame is analytic_kernel.hip's: 16-byte loads and stores, 256 lanes, a grid-stride loop over groups of four elements with a capped
// grid, a lane's NEXT group loaded before the current one is solved.  A vector's storage is a multiple of 256 bytes (Pool::alloc rounds
// the capacity), so the last group is read and written whole: what lies past n is inside the buffer, and every bit pattern is an argument
// the definition takes (its iterations are bounded by FM_IMPLIED_MAX_ITERATIONS whatever the data).  No LDS, no atomics, no inline
// assembly.  The coefficients of Mills' ratio are constants of the code object, read by a piece index that differs between lanes: loads
// from constant memory, no register array is indexed at run time, no scratch.
// Which operands are vectors and which outputs a launch wants is uniform: those branches are scalar.  The partials are evaluated only
// where the mask asks for one (the definition's last step, one fm_option_formula at the root).  A wave pays for its slowest lane: the
// iterations of the definition take about the same handful of steps on every live element, and the degenerate elements none.
// The kernel trusts its arguments: the launcher refuses what implied_shape_ok refuses.
#include <hip/hip_runtime.h>

#include "implied_volatility_kernel.h"

namespace fm {

typedef float iv_f32x4 __attribute__((ext_vector_type(4)));
typedef iv_f32x4 __attribute__((address_space(1))) iv_gfloat4;

template <int MODEL>
__global__ void __launch_bounds__(FM_IMPLIED_BLOCK) fm_implied_volatility_kernel(const DevImpliedArgs A)
{
    using namespace fmhost;
    const int64_t n = A.n;
    const iv_gfloat4* __restrict__ p0 = reinterpret_cast<const iv_gfloat4*>(A.in[0]);
    const iv_gfloat4* __restrict__ p1 = reinterpret_cast<const iv_gfloat4*>(A.in[1]);
    const iv_gfloat4* __restrict__ p2 = reinterpret_cast<const iv_gfloat4*>(A.in[2]);
    const bool v0 = A.in[0] != 0, v1 = A.in[1] != 0, v2 = A.in[2] != 0;
    const bool want_sigma = (A.outputs & FM_IMPLIED_VOLATILITY) != 0, want_d_price = (A.outputs & FM_IMPLIED_D_PRICE) != 0, want_d_forward = (A.outputs & FM_IMPLIED_D_FORWARD) != 0;
    const bool want_partials = want_d_price || want_d_forward;
    const int slot_d_price = want_sigma ? 1 : 0, slot_d_forward = slot_d_price + (want_d_price ? 1 : 0);
    iv_gfloat4* __restrict__ o_sigma = reinterpret_cast<iv_gfloat4*>(A.out[0]);
    iv_gfloat4* __restrict__ o_d_price = reinterpret_cast<iv_gfloat4*>(slot_d_price == 0 ? A.out[0] : A.out[1]);
    iv_gfloat4* __restrict__ o_d_forward = reinterpret_cast<iv_gfloat4*>(slot_d_forward == 0 ? A.out[0] : slot_d_forward == 1 ? A.out[1] : A.out[2]);
    const double root_T = A.root_T, K = A.strike;
    const int64_t stride = (int64_t)gridDim.x * FM_IMPLIED_BLOCK;
    int64_t i4 = (int64_t)blockIdx.x * FM_IMPLIED_BLOCK + threadIdx.x;
    const iv_f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
    iv_f32x4 a0 = zero, a1 = zero, a2 = zero;
    if (i4 * 4 < n) {
        if (v0) a0 = p0[i4];
        if (v1) a1 = p1[i4];
        if (v2) a2 = p2[i4];
    }
#pragma unroll 1
    for (; i4 * 4 < n; i4 += stride) {
        iv_f32x4 c4 = a0, f4 = a1, n4 = a2;
        if ((i4 + stride) * 4 < n) {                                 // the next groups are on their way while these are solved
            if (v0) a0 = p0[i4 + stride];
            if (v1) a1 = p1[i4 + stride];
            if (v2) a2 = p2[i4 + stride];
        }
        iv_f32x4 r_sigma = zero, r_d_price = zero, r_d_forward = zero;
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {                                // rolled: ONE copy of the solver in the code object; the groups rotate through lane x
            const FmImpliedOut r = fm_implied_volatility_masked(MODEL, v0 ? (double)c4.x : A.scalar[0], v1 ? (double)f4.x : A.scalar[1], v2 ? (double)n4.x : A.scalar[2],
                                                                root_T, K, want_partials);
            c4 = c4.yzwx; f4 = f4.yzwx; n4 = n4.yzwx;
            r_sigma = r_sigma.yzwx; r_d_price = r_d_price.yzwx; r_d_forward = r_d_forward.yzwx;
            r_sigma.w = fm_narrow(r.sigma); r_d_price.w = fm_narrow(r.d_price); r_d_forward.w = fm_narrow(r.d_forward);
        }
        if (want_sigma) o_sigma[i4] = r_sigma;
        if (want_d_price) o_d_price[i4] = r_d_price;
        if (want_d_forward) o_d_forward[i4] = r_d_forward;
    }
}

hipError_t launch_implied_volatility(const DevImpliedArgs& a, hipStream_t st)
{
    if (!implied_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(implied_blocks(a.n)), block(FM_IMPLIED_BLOCK);
    if (a.model == (uint32_t)fmhost::FM_FORMULA_BLACK_SCHOLES) hipLaunchKernelGGL(fm_implied_volatility_kernel<fmhost::FM_FORMULA_BLACK_SCHOLES>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(fm_implied_volatility_kernel<fmhost::FM_FORMULA_BACHELIER>, grid, block, 0, st, a);
    return hipGetLastError();
}

} // namespace fm
