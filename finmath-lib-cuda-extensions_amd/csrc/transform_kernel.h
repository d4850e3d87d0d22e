// transform_kernel.h — the host-callable launcher of transform_kernel.hip (engine side: transform_engine.hpp; definition:
// host/transform_formula.hpp): the value per path of a call under a model with an exponential-affine transform, as a finite sum over a node
// table, with its partials in the forward and in the first state; up to four operands that are a vector or a scalar each, up to three outputs.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/transform_formula.hpp"

namespace fm {

constexpr int FM_TRANSFORM_BLOCK = 256;
constexpr int FM_TRANSFORM_TILE = 1024;               // elements per workgroup and iteration: 256 lanes x 16 bytes
constexpr int FM_TRANSFORM_MAX_BLOCKS = 2048;         // the grid's cap: above FM_TRANSFORM_MAX_BLOCKS * FM_TRANSFORM_TILE elements the grid-stride loop wraps
constexpr int FM_TRANSFORM_OPERANDS = 2 + fmhost::FM_TRANSFORM_MAX_STATES;      // forward, payoff unit, the states

struct DevTransformArgs {
    int64_t   n;
    uint32_t  n_nodes, n_states, outputs;              // the mask of FM_TRANSFORM_*
    double    scalar[FM_TRANSFORM_OPERANDS];           // forward, payoff unit, V_0, V_1 where in[k] = 0
    double    strike;
    uint64_t  in[FM_TRANSFORM_OPERANDS];               // an address, or 0: the scalar (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_TRANSFORM_MAX_OUTPUTS];   // one per set bit of outputs, in bit order
    const double* nodes;                               // n_nodes rows of 3 + 2·n_states doubles, on the device
};
inline uint32_t transform_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_TRANSFORM_TILE - 1) / FM_TRANSFORM_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_TRANSFORM_MAX_BLOCKS ? FM_TRANSFORM_MAX_BLOCKS : tiles);
}
inline size_t transform_table_bytes(int n_nodes, int n_states) { return (size_t)n_nodes * (size_t)fmhost::fm_transform_row(n_states) * 8; }
inline bool transform_shape_ok(const DevTransformArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31)) return false;
    if (a.n_nodes < 1 || a.n_nodes > (uint32_t)fmhost::FM_TRANSFORM_MAX_NODES || a.n_states > (uint32_t)fmhost::FM_TRANSFORM_MAX_STATES) return false;
    if (a.outputs < 1 || a.outputs > (uint32_t)fmhost::FM_TRANSFORM_ALL || ((a.outputs & fmhost::FM_TRANSFORM_STATE_DELTA) && a.n_states == 0)) return false;
    if (a.strike != a.strike || !a.nodes) return false;
    bool any = a.in[0] != 0 || a.in[1] != 0;
    for (uint32_t s = 0; s < (uint32_t)fmhost::FM_TRANSFORM_MAX_STATES; ++s) {
        if (s >= a.n_states && a.in[2 + s]) return false;
        any = any || a.in[2 + s] != 0;
    }
    if (!any) return false;
    for (int f = 0; f < fmhost::fm_formula_outputs((int)a.outputs); ++f) if (!a.out[f]) return false;
    return true;
}
hipError_t launch_transform_option(const DevTransformArgs& a, hipStream_t st);

} // namespace fm
