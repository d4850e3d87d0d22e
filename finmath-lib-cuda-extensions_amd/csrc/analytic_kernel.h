// analytic_kernel.h — the host-callable launchers of analytic_kernel.hip (engine side: analytic_engine.hpp; definition:
// host/normal_functions.hpp): named functions of a vector's elements (Φ, φ, Φ⁻¹; up to four per launch, one read of the vector) and the
// option formulas per path (Black–Scholes, Bachelier; up to three operands that are a vector or a scalar each, up to three outputs).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/normal_functions.hpp"

namespace fm {

constexpr int FM_ANALYTIC_BLOCK = 256;
constexpr int FM_ANALYTIC_TILE = 1024;                // elements per workgroup and iteration: 256 lanes x 16 bytes
constexpr int FM_ANALYTIC_MAX_BLOCKS = 2048;          // the grid's cap: above FM_ANALYTIC_MAX_BLOCKS * FM_ANALYTIC_TILE elements the grid-stride loop wraps

struct DevFunctionArgs {
    int64_t   n;
    uint32_t  n_functions, reserved;
    uint32_t  kinds[fmhost::FM_FN_MAX_FUNCTIONS];      // FM_FN_*
    uint64_t  x;                                       // addresses (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_FN_MAX_FUNCTIONS];
};
struct DevFormulaArgs {
    int64_t   n;
    uint32_t  model, outputs;                          // FM_FORMULA_*; the mask
    double    scalar[3];                               // forward, volatility, payoff unit where in[k] = 0
    double    root_T, strike;
    uint64_t  in[3];                                   // an address, or 0: the scalar
    uint64_t  out[fmhost::FM_FORMULA_MAX_OUTPUTS];     // one per set bit of outputs, in bit order
};
inline uint32_t analytic_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_ANALYTIC_TILE - 1) / FM_ANALYTIC_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_ANALYTIC_MAX_BLOCKS ? FM_ANALYTIC_MAX_BLOCKS : tiles);
}
inline bool function_shape_ok(const DevFunctionArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31)) return false;
    if (a.n_functions < 1 || a.n_functions > (uint32_t)fmhost::FM_FN_MAX_FUNCTIONS || !a.x) return false;
    for (uint32_t f = 0; f < a.n_functions; ++f) if (!a.out[f] || a.kinds[f] >= (uint32_t)fmhost::FM_FN_KINDS) return false;
    return true;
}
inline bool formula_shape_ok(const DevFormulaArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31)) return false;
    if (a.model >= (uint32_t)fmhost::FM_FORMULA_MODELS || a.outputs < 1 || a.outputs > (uint32_t)fmhost::FM_FORMULA_ALL) return false;
    if (!(a.root_T >= 0.0) || a.root_T - a.root_T != 0.0 || a.strike - a.strike != 0.0) return false;
    if (!a.in[0] && !a.in[1] && !a.in[2]) return false;
    for (int f = 0; f < fmhost::fm_formula_outputs((int)a.outputs); ++f) if (!a.out[f]) return false;
    return true;
}
hipError_t launch_function_apply(const DevFunctionArgs& a, hipStream_t st);
hipError_t launch_option_formula(const DevFormulaArgs& a, hipStream_t st);

} // namespace fm
