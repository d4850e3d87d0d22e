// xmom_poly_kernel.hip — fm_xmom_poly_kernel and fm_poly_eval_kernel for gfx950 (MI355X, CDNA4): polynomial regression without the basis
// in memory.  DESIGN.md §4.15; contract: include/fmhip.h; definition: host/polynomial_regression.hpp; layout and slots: xmom_poly_kernel.h;
// engine side: xmom_poly_engine.hpp.
//
// fm_xmom_poly_kernel<NG> is fm_xmom_wide_kernel's pass (xmom_wide_device.hpp: the MFMA step, the tree, the arrival) with another way to
// obtain a round's operands.  An ADDRESS slot (an extra regressor, a dependent) is loaded as the wide kernel loads it.  A TERM slot is
// formed by its lane: the lane (sub = lane >> 4) loads the four paths of its round of every state vector with one 16-byte load — the 16
// lanes of a sub-index read the same address, which is one request —, builds the powers u, u·u, (u·u)·u … of the state once per round
// (they are the same for the lane's term of every group) and, per group, SELECTS the power its exponent asks for, 1.0f for exponent 0,
// and multiplies it on: t = t·sel, from t = 1.0f.  x·1.0f is x for every x, so this is the chain of the contract — the powers in ascending
// state index, left to right, a state with exponent 0 not taking part (inf⁰ never meets a 0) — without a lane-divergent branch.  The
// loop over the powers ends at the largest exponent of the call, and groups without a term skip the arithmetic: both wave-uniform.
// Paths past n are zeroed AFTER the term is formed: a product of garbage is replaced, never multiplied by 0.
// State loads are double-buffered round by round with the address slots; no register array is indexed at run time: no scratch.
//
// fm_poly_eval_kernel: one lane per four paths; exponents and coefficients are kernel arguments read with wave-uniform indices, so a
// term's chain is straight-line scalar-controlled code.  -ffp-contract=off: no product meets a sum in an fma.
#include <hip/hip_runtime.h>

#include "xmom_poly_kernel.h"
#include "xmom_wide_device.hpp"

namespace fm {

template <int NG>
struct XwPolyRaw {
    XwRound<NG> v;                                                  // address slots (terms: +0.0 so far)
    xw_f32x4 st[FM_POLY_MAX_STATES];
};

template <int NG>
struct XwPolyPolicy {
    typedef XwPolyRaw<NG> Raw;
    XwAddressLoads<NG, true> a;
    uint64_t state[FM_POLY_MAX_STATES];                             // wave-uniform
    uint32_t n_states, max_exponent;
    int64_t n;
    uint32_t sub;
    uint32_t exps[NG];                                              // this lane's term of group g: 8 x 3 bits; 0: not a term
    bool group_has_term[NG];                                        // wave-uniform

    __device__ __forceinline__ void init(const uint64_t* slots, const uint32_t lane, const uint32_t sub_)
    {
        sub = sub_;
        a.init(slots, lane, sub_);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const uint64_t slot = slots[g * FM_XMOMW_GROUP + (lane & 15u)];
            exps[g] = (slot & FM_XMOMW_TERM) ? (uint32_t)slot & 0xffffffu : 0u;
            group_has_term[g] = __ballot(exps[g] != 0u) != 0ull;
        }
    }
    __device__ __forceinline__ void load(const uint32_t c, const int r, Raw& k) const
    {
        a.load(c, r, k.v);
        const uint64_t at = (uint64_t)c * (FM_XMOMW_CHUNK * 4) + (uint64_t)r * 64u + sub * 16u;
#pragma unroll
        for (int s = 0; s < FM_POLY_MAX_STATES; ++s)
            if ((uint32_t)s < n_states) k.st[s] = *reinterpret_cast<const xw_gfloat4*>(state[s] + at);
    }
    __device__ __forceinline__ void form(const uint32_t c, const int r, const Raw& k, XwRound<NG>& o) const
    {
        const xw_f32x4 ones = { 1.0f, 1.0f, 1.0f, 1.0f };
        xw_f32x4 t[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) t[g] = ones;
#pragma unroll
        for (int s = 0; s < FM_POLY_MAX_STATES; ++s) {
            if ((uint32_t)s >= n_states) break;
            const xw_f32x4 u = k.st[s];
            xw_f32x4 pw[FM_POLY_MAX_EXPONENT];                      // pw[j] = u^(j+1): ((u·u)·u)…
            pw[0] = u;
#pragma unroll
            for (int j = 1; j < FM_POLY_MAX_EXPONENT; ++j) { pw[j] = pw[j - 1]; if ((uint32_t)j < max_exponent) pw[j] = pw[j - 1] * u; }
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                if (!group_has_term[g]) continue;
                const uint32_t e = (exps[g] >> (3 * s)) & 7u;
                xw_f32x4 sel = e >= 1u ? pw[0] : ones;
#pragma unroll
                for (int j = 1; j < FM_POLY_MAX_EXPONENT; ++j)
                    if ((uint32_t)j < max_exponent) sel = e >= (uint32_t)(j + 1) ? pw[j] : sel;
                t[g] = t[g] * sel;
            }
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) o.v[g] = exps[g] != 0u ? t[g] : k.v.v[g];
        xw_zero_tail<NG>(o, (int64_t)c * FM_XMOMW_CHUNK + r * 16 + sub * 4u, n);
    }
};

template <int NG>
__global__ void __launch_bounds__(FM_XMOMW_BLOCK) fm_xmom_poly_kernel(const DevXmomPolyArgs A)
{
    XwPolyPolicy<NG> P;
#pragma unroll
    for (int s = 0; s < FM_POLY_MAX_STATES; ++s) P.state[s] = A.state[s];
    P.n_states = A.n_states; P.max_exponent = A.max_exponent; P.n = A.w.n;
    xw_pass<NG>(A.w, P);
}

__global__ void __launch_bounds__(FM_POLY_EVAL_BLOCK) fm_poly_eval_kernel(const DevPolyEvalArgs A)
{
    const int64_t n = A.n;
    const uint32_t ns = A.n_states, nt = A.n_terms, ne = A.n_extra;
    const xw_f32x4 ones = { 1.0f, 1.0f, 1.0f, 1.0f };
    xw_gfloat4* __restrict__ po = reinterpret_cast<xw_gfloat4*>(A.out);
#pragma unroll 1
    for (int64_t i4 = (int64_t)blockIdx.x * FM_POLY_EVAL_BLOCK + threadIdx.x; i4 * 4 < n; i4 += (int64_t)gridDim.x * FM_POLY_EVAL_BLOCK) {
        xw_f32x4 st[FM_POLY_MAX_STATES];
#pragma unroll
        for (int s = 0; s < FM_POLY_MAX_STATES; ++s)
            if ((uint32_t)s < ns) st[s] = reinterpret_cast<const xw_gfloat4*>(A.state[s])[i4];
        xw_f32x4 r = ones;
#pragma unroll 1
        for (uint32_t i = 0; i < nt; ++i) {                         // i, the exponents and the coefficient are wave-uniform
            const uint32_t ex = A.exponents[i];
            const float c = A.coefficient[i];
            xw_f32x4 t = ones;
            bool started = false;
#pragma unroll
            for (int s = 0; s < FM_POLY_MAX_STATES; ++s) {
                if ((uint32_t)s >= ns) break;
                const uint32_t e = (ex >> (3 * s)) & 7u;
                if (e == 0u) continue;
                xw_f32x4 p = st[s];
#pragma unroll 1
                for (uint32_t j = 1; j < e; ++j) p = p * st[s];
                t = started ? t * p : p;
                started = true;
            }
            const xw_f32x4 tc = t * c;
            r = i == 0u ? tc : r + tc;
        }
#pragma unroll 1
        for (uint32_t j = 0; j < ne; ++j) {
            const uint64_t at = A.extra[j];
            const xw_f32x4 x = at ? reinterpret_cast<const xw_gfloat4*>(at)[i4] : ones;
            r = r + x * A.coefficient[nt + j];
        }
        po[i4] = r;
    }
}

hipError_t launch_xmom_poly(const DevXmomPolyArgs& a, hipStream_t st)
{
    if (!xmom_poly_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(xmom_wide_blocks(a.w.n), 1, 1), block(FM_XMOMW_BLOCK);
    switch (a.w.n_groups) {
    case 1:  hipLaunchKernelGGL(fm_xmom_poly_kernel<1>, grid, block, 0, st, a); break;
    case 2:  hipLaunchKernelGGL(fm_xmom_poly_kernel<2>, grid, block, 0, st, a); break;
    case 3:  hipLaunchKernelGGL(fm_xmom_poly_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(fm_xmom_poly_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_poly_eval(const DevPolyEvalArgs& a, hipStream_t st)
{
    if (!poly_eval_shape_ok(a)) return hipErrorInvalidValue;
    int64_t blocks = (a.n + 4 * FM_POLY_EVAL_BLOCK - 1) / (4 * FM_POLY_EVAL_BLOCK);
    if (blocks > FM_POLY_EVAL_MAX_BLOCKS) blocks = FM_POLY_EVAL_MAX_BLOCKS;
    hipLaunchKernelGGL(fm_poly_eval_kernel, dim3((uint32_t)blocks), dim3(FM_POLY_EVAL_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
