// transform_engine.hpp — the engine's side of the transform option value per path (kernel: transform_kernel.hip;
// definition and argument check: host/transform_formula.hpp).  A producing pass in the frame of side_pass_engine.hpp (which says what every
// such pass does), beside the option formulas of analytic_engine.hpp.
//
// transform_option: value (and, by a mask, ∂/∂forward and ∂/∂V_0) of a call under a model whose transform is exponential-affine in up to two
// states, as the finite sum over a node table; forward, payoff unit and the states are each a vector or a scalar; one new vector per set
// bit.  The node table goes up in ONE in-stream copy from the pinned stage that the host waits for (the staging block is the engine's: it
// must be free again when the call returns), as Engine::table_apply's coefficients do; the launch itself is not waited for.  The pass is
// elementwise: a device list runs it per shard (sharded.cpp), a communicator's ranks each on their own paths.
#include "runtime.hpp"
#include "transform_kernel.h"

#include <cstring>

namespace fm {

static_assert(FMHIP_TRANSFORM_VALUE == fmhost::FM_TRANSFORM_VALUE && FMHIP_TRANSFORM_DELTA == fmhost::FM_TRANSFORM_DELTA
              && FMHIP_TRANSFORM_STATE_DELTA == fmhost::FM_TRANSFORM_STATE_DELTA && FMHIP_TRANSFORM_MAX_NODES == fmhost::FM_TRANSFORM_MAX_NODES
              && FMHIP_TRANSFORM_MAX_STATES == fmhost::FM_TRANSFORM_MAX_STATES,
              "include/fmhip.h and host/transform_formula.hpp name the same outputs and limits");

// WEAK: see pass_need_kernel (tests/nulldev/null_transform.cpp has the stand-in).
hipError_t launch_transform_option(const DevTransformArgs& a, hipStream_t st) __attribute__((weak));

void transform_check(const double* nodes, int n_nodes, int n_states, fmhip_vec forward, const fmhip_vec* states, const double* state_scalars, fmhip_vec payoff_unit,
                     double strike, int outputs, const fmhip_vec* out) {
    bool any_vector = forward != 0 || payoff_unit != 0;
    if (states && n_states >= 0 && n_states <= fmhost::FM_TRANSFORM_MAX_STATES) for (int s = 0; s < n_states; ++s) any_vector = any_vector || states[s] != 0;
    pass_as_engine_error([&] { fmhost::transformCheck(nodes, n_nodes, n_states, states, state_scalars, any_vector, strike, outputs, out); });
}
// fmhip_transform_option_host: the definition, with its complaints as engine errors
void transform_option_host_checked(const double* nodes, int n_nodes, int n_states, const float* forward, double forward_scalar, const float* const* states,
                                   const double* state_scalars, const float* payoff_unit, double payoff_unit_scalar, int64_t n, double strike, int outputs, float* const* out) {
    pass_as_engine_error([&] { fmhost::transform_option_host(nodes, n_nodes, n_states, forward, forward_scalar, states, state_scalars, payoff_unit, payoff_unit_scalar, n, strike, outputs, out); });
}

void Engine::transform_option(const double* nodes, int n_nodes, int n_states, fmhip_vec forward, double forward_scalar, const fmhip_vec* states,
                              const double* state_scalars, fmhip_vec payoff_unit, double payoff_unit_scalar, double strike, int outputs, fmhip_vec* out) {
    require_init();
    transform_check(nodes, n_nodes, n_states, forward, states, state_scalars, payoff_unit, strike, outputs, out);
    fmhip_vec operands[FM_TRANSFORM_OPERANDS] = { forward, payoff_unit, 0, 0 };
    for (int s = 0; s < n_states; ++s) operands[2 + s] = states[s];
    fmhip_vec vectors[FM_TRANSFORM_OPERANDS]; int slot[FM_TRANSFORM_OPERANDS]; int n_vectors = 0;
    for (int k = 0; k < FM_TRANSFORM_OPERANDS; ++k) if (operands[k]) { vectors[n_vectors] = operands[k]; slot[n_vectors++] = k; }
    pass_size(vectors, n_vectors, "transform option");
    pass_need_kernel(launch_transform_option != nullptr, "transform-option");
    PassHold hold;
    pass_prepare(vectors, n_vectors, hold, "transform option");
    const int n_out = fmhost::fm_formula_outputs(outputs);
    DevTransformArgs a{};
    a.n = hold.n; a.n_nodes = (uint32_t)n_nodes; a.n_states = (uint32_t)n_states; a.outputs = (uint32_t)outputs;
    a.scalar[0] = forward_scalar; a.scalar[1] = payoff_unit_scalar;
    for (int s = 0; s < n_states; ++s) a.scalar[2 + s] = state_scalars[s];
    a.strike = strike;
    for (int v = 0; v < n_vectors; ++v) a.in[slot[v]] = hold.ptrs[(size_t)v];
    PassOutputs outs(this);
    for (int f = 0; f < n_out; ++f) a.out[f] = outs.add(hold.n);
    // the node table goes up in one copy; the copy has left the pinned block before this call returns
    const size_t table_bytes = transform_table_bytes(n_nodes, n_states);
    char* stage = (char*)ensure_stage(table_bytes);
    pass_scratch(pass_up256(8), table_bytes);
    std::memcpy(stage, nodes, table_bytes);
    hip_check(hipMemcpyAsync(pass_other_, stage, table_bytes, hipMemcpyHostToDevice, stream_), "H2D(node table)");
    hip_check(hipStreamSynchronize(stream_), "sync");
    a.nodes = (const double*)pass_other_;
    hip_check(launch_transform_option(a, stream_), "launch fm_transform_option_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_vectors + n_out);
    bytes_written_ += 4 * hold.n * n_out;
    outs.commit(out);
}

} // namespace fm
