// transform_kernel.hip — fm_transform_option_kernel for gfx950 (MI355X, CDNA4): the value per path of a call under a model whose transform
// is exponential-affine in up to two states (Black–Scholes, Merton, Heston, Bates, double Heston), with ∂/∂forward and ∂/∂V_0, as the
// finite sum over a node table.  DESIGN.md §4.28; contract: include/fmhip.h; definition: host/transform_formula.hpp (the function evaluated
// here is ITS function — fm_transform_open, fm_transform_node, fm_transform_close — compiled for the device: + − × /, sqrt, comparisons and
// integer operations in fp64, no contraction — the bits are the host's); engine side: transform_engine.hpp.
//
// The frame is analytic_kernel.hip's: 16-byte loads and stores, 256 lanes, a grid-stride loop over groups of four elements with a capped
// grid, a lane's NEXT group loaded before the current one is summed.  A vector's storage is a multiple of 256 bytes (Pool::alloc rounds
// the capacity), so the last group is read and written whole: what lies past n is inside the buffer, and every bit pattern is an argument
// the definition takes.  The node loop runs OUTSIDE the group's four elements: a node's row is fetched once per group, and the four
// exp/sincos chains of a node are independent of each other.  The row's index is the same in every lane and the table's pointer is a kernel
// argument: the rows come through scalar loads, no LDS.  An element that the definition closes before its sum (a NaN operand, F or K not
// positive) runs through the nodes with k = 0 like its neighbours — no lane waits for another — and takes the closed result at the end.
// The group's per-element values are named by unrolled constant indices: registers, no array indexed at run time, no scratch.  No atomics,
// no inline assembly.  The constants of fm_exp64, fm_log64 and fm_sincos64 are literals of the code object.
// Which operands are vectors and which outputs a launch wants is uniform: those branches are scalar.
// The kernel trusts its arguments: the launcher refuses what transform_shape_ok refuses.
#include <hip/hip_runtime.h>

#include "transform_kernel.h"

namespace fm {

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));
typedef tr_f32x4 __attribute__((address_space(1))) tr_gfloat4;

template <int S>
__global__ void __launch_bounds__(FM_TRANSFORM_BLOCK) fm_transform_option_kernel(const DevTransformArgs A, const double* __restrict__ nodes)
{
    using namespace fmhost;
    constexpr int ROW = 3 + 2 * S;
    const int64_t n = A.n;
    const tr_gfloat4* __restrict__ p0 = reinterpret_cast<const tr_gfloat4*>(A.in[0]);
    const tr_gfloat4* __restrict__ p1 = reinterpret_cast<const tr_gfloat4*>(A.in[1]);
    const tr_gfloat4* __restrict__ p2 = reinterpret_cast<const tr_gfloat4*>(A.in[2]);
    const tr_gfloat4* __restrict__ p3 = reinterpret_cast<const tr_gfloat4*>(A.in[3]);
    const bool v0 = A.in[0] != 0, v1 = A.in[1] != 0, v2 = S >= 1 && A.in[2] != 0, v3 = S >= 2 && A.in[3] != 0;
    const bool want_value = (A.outputs & FM_TRANSFORM_VALUE) != 0, want_delta = (A.outputs & FM_TRANSFORM_DELTA) != 0, want_state = (A.outputs & FM_TRANSFORM_STATE_DELTA) != 0;
    const int slot_delta = want_value ? 1 : 0, slot_state = slot_delta + (want_delta ? 1 : 0);
    tr_gfloat4* __restrict__ o_value = reinterpret_cast<tr_gfloat4*>(A.out[0]);
    tr_gfloat4* __restrict__ o_delta = reinterpret_cast<tr_gfloat4*>(slot_delta == 0 ? A.out[0] : A.out[1]);
    tr_gfloat4* __restrict__ o_state = reinterpret_cast<tr_gfloat4*>(slot_state == 0 ? A.out[0] : slot_state == 1 ? A.out[1] : A.out[2]);
    const int J = (int)A.n_nodes;
    const double K = A.strike;
    const int64_t stride = (int64_t)gridDim.x * FM_TRANSFORM_BLOCK;
    int64_t i4 = (int64_t)blockIdx.x * FM_TRANSFORM_BLOCK + threadIdx.x;
    const tr_f32x4 zero = { 0.0f, 0.0f, 0.0f, 0.0f };
    tr_f32x4 a0 = zero, a1 = zero, a2 = zero, a3 = zero;
    if (i4 * 4 < n) {
        if (v0) a0 = p0[i4];
        if (v1) a1 = p1[i4];
        if (v2) a2 = p2[i4];
        if (v3) a3 = p3[i4];
    }
#pragma unroll 1
    for (; i4 * 4 < n; i4 += stride) {
        const tr_f32x4 f4 = a0, n4 = a1, s4 = a2, t4 = a3;
        if ((i4 + stride) * 4 < n) {                                 // the next groups are on their way while these are summed
            if (v0) a0 = p0[i4 + stride];
            if (v1) a1 = p1[i4 + stride];
            if (v2) a2 = p2[i4 + stride];
            if (v3) a3 = p3[i4 + stride];
        }
        double F[4], N[4], V0[4], V1[4], k[4];
        bool open[4];
        FmTransformOut closed[4];
        FmTransformSums sums[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            F[e] = v0 ? (double)f4[e] : A.scalar[0];
            N[e] = v1 ? (double)n4[e] : A.scalar[1];
            V0[e] = v2 ? (double)s4[e] : A.scalar[2];
            V1[e] = v3 ? (double)t4[e] : A.scalar[3];
            k[e] = 0.0;
            closed[e].value = closed[e].delta = closed[e].state_delta = 0.0;
            open[e] = fm_transform_open(S, F[e], N[e], V0[e], V1[e], K, k[e], closed[e]);
            sums[e].G = sums[e].H = sums[e].GV = 0.0;
        }
#pragma unroll 1
        for (int j = 0; j < J; ++j) {
            const double* __restrict__ row = nodes + j * ROW;         // uniform: one fetch per group
#pragma unroll
            for (int e = 0; e < 4; ++e) fm_transform_node<S>(row, k[e], V0[e], V1[e], sums[e]);
        }
        tr_f32x4 r_value = zero, r_delta = zero, r_state = zero;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const FmTransformOut live = fm_transform_close(F[e], N[e], K, sums[e]);
            r_value[e] = fm_narrow(open[e] ? live.value : closed[e].value);
            r_delta[e] = fm_narrow(open[e] ? live.delta : closed[e].delta);
            r_state[e] = fm_narrow(open[e] ? live.state_delta : closed[e].state_delta);
        }
        if (want_value) o_value[i4] = r_value;
        if (want_delta) o_delta[i4] = r_delta;
        if (want_state) o_state[i4] = r_state;
    }
}

hipError_t launch_transform_option(const DevTransformArgs& a, hipStream_t st)
{
    if (!transform_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(transform_blocks(a.n)), block(FM_TRANSFORM_BLOCK);
    if (a.n_states == 0) hipLaunchKernelGGL(fm_transform_option_kernel<0>, grid, block, 0, st, a, a.nodes);
    else if (a.n_states == 1) hipLaunchKernelGGL(fm_transform_option_kernel<1>, grid, block, 0, st, a, a.nodes);
    else hipLaunchKernelGGL(fm_transform_option_kernel<2>, grid, block, 0, st, a, a.nodes);
    return hipGetLastError();
}

} // namespace fm
