// implied_volatility_kernel.h — the host-callable launcher of implied_volatility_kernel.hip (engine side:
// implied_volatility_engine.hpp; definition: host/implied_volatility.hpp): the implied volatility per path of a Black–Scholes or Bachelier
// call price, with its partials in the price and the forward; three operands that are a vector or a scalar each, up to three outputs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/implied_volatility.hpp"

namespace fm {

constexpr int FM_IMPLIED_BLOCK = 256;
constexpr int FM_IMPLIED_TILE = 1024;                 // elements per workgroup and iteration: 256 lanes x 16 bytes
constexpr int FM_IMPLIED_MAX_BLOCKS = 2048;           // the grid's cap: above FM_IMPLIED_MAX_BLOCKS * FM_IMPLIED_TILE elements the grid-stride loop wraps

struct DevImpliedArgs {
    int64_t   n;
    uint32_t  model, outputs;                          // FM_FORMULA_*; the mask of FM_IMPLIED_*
    double    scalar[3];                               // price, forward, payoff unit where in[k] = 0
    double    root_T, strike;
    uint64_t  in[3];                                   // an address, or 0: the scalar (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_IMPLIED_MAX_OUTPUTS];     // one per set bit of outputs, in bit order
};
inline uint32_t implied_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_IMPLIED_TILE - 1) / FM_IMPLIED_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_IMPLIED_MAX_BLOCKS ? FM_IMPLIED_MAX_BLOCKS : tiles);
}
inline bool implied_shape_ok(const DevImpliedArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31)) return false;
    if (a.model >= (uint32_t)fmhost::FM_FORMULA_MODELS || a.outputs < 1 || a.outputs > (uint32_t)fmhost::FM_IMPLIED_ALL) return false;
    if (!(a.root_T >= 0.0) || a.root_T - a.root_T != 0.0 || a.strike - a.strike != 0.0) return false;
    if (!a.in[0] && !a.in[1] && !a.in[2]) return false;
    for (int f = 0; f < fmhost::fm_formula_outputs((int)a.outputs); ++f) if (!a.out[f]) return false;
    return true;
}
hipError_t launch_implied_volatility(const DevImpliedArgs& a, hipStream_t st);

} // namespace fm
