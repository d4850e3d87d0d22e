// transform_formula.hpp — the definition of the TRANSFORM OPTION VALUE per path: a call in forward form under a model whose characteristic
// function is exponential-affine in at most two state variables (Black–Scholes and Merton: none; Heston and Bates: the variance; double
// Heston: two), as the finite sum that a fixed quadrature of Lewis' single integral leaves, in ONE header that the host (g++, hipcc -x c++)
// and the device (csrc/transform_kernel.hip) both compile.  DESIGN.md §4.28; contract: include/fmhip.h.
//
// The rules are normal_functions.hpp's: fp64, only + − × /, __builtin_sqrt, comparisons and integer operations, fm_exp64, fm_log64 and
// fm_sincos64 (trig64.hpp); every operation rounded once by IEEE 754 on either side (builds: -ffp-contract=off, no fast-math); no <cmath>
// transcendental, no OCML call.  What the device computes EQUALS what the host does.
//
// THE NODE TABLE: J rows (1 … FM_TRANSFORM_MAX_NODES), S state variables (0 … FM_TRANSFORM_MAX_STATES); row j holds 3 + 2S doubles
//     u_j, a_re, a_im, b_re[0..S), b_im[0..S)
// computed by the caller once (transform.py: C(u) and D(u) of the model in complex arithmetic, the quadrature weight folded into a_re as its
// logarithm).  The nodes are data to this header: which rule they come from is the caller's business.
//
// OPERANDS: forward F, payoff unit N and the states V_0 … V_{S−1}, each a vector (the (double) of its fp32 elements) or an fp64 scalar; the
// strike K an fp64 scalar.  PER ELEMENT, every operation on its own, left to right:
//     a NaN among F, N, V_s, K                      the quiet NaN in every output
//     not (F > 0 and K > 0)                         fm_option_formula's limit: value N·max(F − K, 0), delta N·[F > K], state partial 0
//     otherwise, k = fm_log64(F / K), G = H = GV = 0, and for j = 0 … J−1 in this order
//         e = a_re + Σ_s b_re[s]·V_s                θ = a_im + Σ_s b_im[s]·V_s + u_j·k
//         E = fm_exp64(e)                           (s, c) = fm_sincos64(θ)
//         G += E·c        H −= (E·u_j)·s            GV += E·(b_re[0]·c − b_im[0]·s)          (GV for S >= 1)
//     root = __builtin_sqrt(F·K)
//         value          N·(F − root·G)
//         delta  ∂/∂F    N·(1 − (root/F)·(0.5·G + H))
//         state  ∂/∂V_0  N·(0 − root·GV)                                                     (needs S >= 1)
// NOTHING IS CLAMPED: the value is not forced into the arbitrage bounds; an e that overflows or a θ beyond FM_TRIG_MAX gives whatever IEEE
// 754 and fm_sincos64 give — a NaN (∞·c with c = 0, ∞ − ∞, or the sine of an argument out of range), which comes back as the quiet NaN
// 0x7fc00000 — or an infinity.  Results are narrowed once (fm_narrow).
// Host only, below: transform_option_host (the definition over arrays) and its argument check, which complain with std::invalid_argument.
#pragma once
#include <stdint.h>

#include "normal_functions.hpp"
#include "trig64.hpp"

namespace fmhost {

enum { FM_TRANSFORM_VALUE = 1, FM_TRANSFORM_DELTA = 2, FM_TRANSFORM_STATE_DELTA = 4, FM_TRANSFORM_ALL = 7 };      // = FMHIP_TRANSFORM_*
constexpr int FM_TRANSFORM_MAX_OUTPUTS = 3;
constexpr int FM_TRANSFORM_MAX_NODES = 256;
constexpr int FM_TRANSFORM_MAX_STATES = 2;
FM_HD inline int fm_transform_row(int S) { return 3 + 2 * S; }      // doubles of a node's row

struct FmTransformSums { double G, H, GV; };
struct FmTransformOut { double value, delta, state_delta; };

// one node's terms added to the sums of one element; V1 is read for S = 2 only, V0 for S >= 1
template <int S>
FM_HD inline __attribute__((always_inline)) void fm_transform_node(const double* row, double k, double V0, double V1, FmTransformSums& sums)
{
    const double u = row[0];
    double e = row[1], theta = row[2];
    if (S >= 1) { e = e + row[3] * V0; theta = theta + row[3 + S] * V0; }
    if (S >= 2) { e = e + row[4] * V1; theta = theta + row[4 + S] * V1; }
    theta = theta + u * k;
    const double E = fm_exp64(e);
    const FmSinCos sc = fm_sincos64(theta);
    sums.G = sums.G + E * sc.cos;
    sums.H = sums.H - (E * u) * sc.sin;
    if (S >= 1) sums.GV = sums.GV + E * (row[3] * sc.cos - row[3 + S] * sc.sin);
}

// the element's class before any node is looked at: true = the sums are wanted (k is set); false = out is final
FM_HD inline __attribute__((always_inline)) bool fm_transform_open(int S, double F, double N, double V0, double V1, double K, double& k, FmTransformOut& out)
{
    if (F != F || N != N || K != K || (S >= 1 && V0 != V0) || (S >= 2 && V1 != V1)) {
        out.value = out.delta = out.state_delta = fm_double(0x7ff8000000000000ull);
        return false;
    }
    if (!(F > 0.0 && K > 0.0)) {
        const double intrinsic = F - K;
        out.value = N * (intrinsic > 0.0 ? intrinsic : 0.0);
        out.delta = N * (F > K ? 1.0 : 0.0);
        out.state_delta = 0.0;
        return false;
    }
    k = fm_log64(F / K);
    return true;
}
FM_HD inline __attribute__((always_inline)) FmTransformOut fm_transform_close(double F, double N, double K, const FmTransformSums& sums)
{
    FmTransformOut out;
    const double root = __builtin_sqrt(F * K);
    out.value = N * (F - root * sums.G);
    out.delta = N * (1.0 - (root / F) * (0.5 * sums.G + sums.H));
    out.state_delta = N * (0.0 - root * sums.GV);
    return out;
}

template <int S>
FM_HD inline FmTransformOut fm_transform_option_s(const double* nodes, int J, double F, double N, double V0, double V1, double K)
{
    FmTransformOut out;
    double k = 0.0;
    if (!fm_transform_open(S, F, N, V0, V1, K, k, out)) return out;
    FmTransformSums sums; sums.G = sums.H = sums.GV = 0.0;
    for (int j = 0; j < J; ++j) fm_transform_node<S>(nodes + (int64_t)j * (3 + 2 * S), k, V0, V1, sums);
    return fm_transform_close(F, N, K, sums);
}
FM_HD inline FmTransformOut fm_transform_option(const double* nodes, int J, int S, double F, double N, double V0, double V1, double K)
{
    return S == 0 ? fm_transform_option_s<0>(nodes, J, F, N, V0, V1, K) : S == 1 ? fm_transform_option_s<1>(nodes, J, F, N, V0, V1, K)
                                                                                  : fm_transform_option_s<2>(nodes, J, F, N, V0, V1, K);
}

} // namespace fmhost

// ---------------------------------------------------------------- host only: the argument check and the definition over arrays
#if !defined(__HIP_DEVICE_COMPILE__)
namespace fmhost {

// what can be said about fmhip_transform_option's arguments without looking at a vector; any_vector: one operand at least is a vector
inline void transformCheck(const double* nodes, int n_nodes, int n_states, const void* states, const double* state_scalars, bool any_vector, double strike, int outputs, const void* out)
{
    if (n_nodes < 1 || n_nodes > FM_TRANSFORM_MAX_NODES) throw std::invalid_argument("transform option: " + std::to_string(n_nodes) + " nodes (1 … 256)");
    if (n_states < 0 || n_states > FM_TRANSFORM_MAX_STATES) throw std::invalid_argument("transform option: " + std::to_string(n_states) + " state variables (0 … 2)");
    if (outputs < 1 || outputs > FM_TRANSFORM_ALL) throw std::invalid_argument("transform option: outputs is a mask of value (1), delta (2) and state delta (4)");
    if ((outputs & FM_TRANSFORM_STATE_DELTA) && n_states == 0) throw std::invalid_argument("transform option: the state delta needs a state variable");
    if (!nodes) throw std::invalid_argument("transform option: null pointer: nodes");
    if (n_states > 0 && !states) throw std::invalid_argument("transform option: null pointer: states");
    if (n_states > 0 && !state_scalars) throw std::invalid_argument("transform option: null pointer: state_scalars");
    if (!out) throw std::invalid_argument("transform option: null pointer: out");
    const int entries = n_nodes * fm_transform_row(n_states);
    for (int i = 0; i < entries; ++i)
        if (nodes[i] - nodes[i] != 0.0) throw std::invalid_argument("transform option: the node table's entry " + std::to_string(i) + " is not finite");
    if (!any_vector) throw std::invalid_argument("transform option: at least one of forward, states and payoff unit is a vector");
    if (strike != strike) throw std::invalid_argument("transform option: the strike is a NaN");
}

// forward, states[s], payoff_unit: an array of n floats, or NULL for the scalar beside it; out: one array per set bit of outputs, in bit order
inline void transform_option_host(const double* nodes, int n_nodes, int n_states, const float* forward, double forward_scalar, const float* const* states,
                                  const double* state_scalars, const float* payoff_unit, double payoff_unit_scalar, int64_t n, double strike, int outputs, float* const* out)
{
    bool any_vector = forward != nullptr || payoff_unit != nullptr;
    if (states && n_states >= 0 && n_states <= FM_TRANSFORM_MAX_STATES) for (int s = 0; s < n_states; ++s) any_vector = any_vector || states[s] != nullptr;
    transformCheck(nodes, n_nodes, n_states, states, state_scalars, any_vector, strike, outputs, out);
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("transform option: of " + std::to_string(n) + " elements (1 … 2^31)");
    const int n_out = fm_formula_outputs(outputs);
    for (int f = 0; f < n_out; ++f) if (!out[f]) throw std::invalid_argument("transform option: null pointer: out[" + std::to_string(f) + "]");
    const float* v[FM_TRANSFORM_MAX_STATES] = { nullptr, nullptr };
    double vs[FM_TRANSFORM_MAX_STATES] = { 0.0, 0.0 };
    for (int s = 0; s < n_states; ++s) { v[s] = states[s]; vs[s] = state_scalars[s]; }
    for (int64_t p = 0; p < n; ++p) {
        const FmTransformOut r = fm_transform_option(nodes, n_nodes, n_states, forward ? (double)forward[p] : forward_scalar, payoff_unit ? (double)payoff_unit[p] : payoff_unit_scalar,
                                                     v[0] ? (double)v[0][p] : vs[0], v[1] ? (double)v[1][p] : vs[1], strike);
        int f = 0;
        if (outputs & FM_TRANSFORM_VALUE) out[f++][p] = fm_narrow(r.value);
        if (outputs & FM_TRANSFORM_DELTA) out[f++][p] = fm_narrow(r.delta);
        if (outputs & FM_TRANSFORM_STATE_DELTA) out[f++][p] = fm_narrow(r.state_delta);
    }
}

} // namespace fmhost
#endif
