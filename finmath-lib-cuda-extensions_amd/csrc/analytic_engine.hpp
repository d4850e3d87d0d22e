// analytic_engine.hpp — the engine's side of the named functions and the option formulas per path (kernels:
// analytic_kernel.hip; definition and argument checks: host/normal_functions.hpp).  Producing passes in the frame of side_pass_engine.hpp
// (which says what every such pass does).
//
// function_apply: up to four of Φ, φ, Φ⁻¹ applied to every element of x, each result a new vector.  option_formula: value, delta and vega
// (any of them, by a mask) of a Black–Scholes or Bachelier call whose forward, volatility and payoff unit are each a vector or a scalar;
// one new vector per set bit.  Both: one launch, not waited for; nothing goes through the pinned stage — the arguments are the launch's.
// The passes are elementwise: a device list runs them per shard (sharded.cpp), a communicator's ranks each on their own paths.
#include "runtime.hpp"
#include "analytic_kernel.h"

namespace fm {

static_assert(FMHIP_FN_NORMAL_CDF == fmhost::FM_FN_NORMAL_CDF && FMHIP_FN_NORMAL_DENSITY == fmhost::FM_FN_NORMAL_DENSITY
              && FMHIP_FN_NORMAL_QUANTILE == fmhost::FM_FN_NORMAL_QUANTILE && FMHIP_FORMULA_BLACK_SCHOLES == fmhost::FM_FORMULA_BLACK_SCHOLES
              && FMHIP_FORMULA_BACHELIER == fmhost::FM_FORMULA_BACHELIER && FMHIP_FORMULA_VALUE == fmhost::FM_FORMULA_VALUE
              && FMHIP_FORMULA_DELTA == fmhost::FM_FORMULA_DELTA && FMHIP_FORMULA_VEGA == fmhost::FM_FORMULA_VEGA,
              "include/fmhip.h and host/normal_functions.hpp name the same functions, models and outputs");

// WEAK: see pass_need_kernel (tests/nulldev/null_analytic.cpp has the stand-ins).
hipError_t launch_function_apply(const DevFunctionArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_option_formula(const DevFormulaArgs& a, hipStream_t st) __attribute__((weak));

void analytic_check_function(fmhip_vec x, const int* kinds, int n_functions, const fmhip_vec* out) {
    if (!x) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "named functions: of a vector");
    pass_as_engine_error([&] { fmhost::functionCheckApply(kinds, n_functions, out); });
}
void analytic_check_formula(int model, fmhip_vec forward, fmhip_vec volatility, fmhip_vec payoff_unit, double maturity, double strike, int outputs, const fmhip_vec* out) {
    pass_as_engine_error([&] { fmhost::formulaCheck(model, maturity, strike, outputs, out); });
    if (!forward && !volatility && !payoff_unit) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "option formula: at least one of forward, volatility and payoff unit is a vector");
}
// fmhip_function_apply_host and fmhip_option_formula_host: the definitions, with their complaints as engine errors
void function_apply_host_checked(const float* x, int64_t n, const int* kinds, int n_functions, float* const* out) {
    pass_as_engine_error([&] { fmhost::function_apply_host(x, n, kinds, n_functions, out); });
}
void option_formula_host_checked(int model, const float* forward, double forward_scalar, const float* volatility, double volatility_scalar, const float* payoff_unit,
                                 double payoff_unit_scalar, int64_t n, double maturity, double strike, int outputs, float* const* out) {
    pass_as_engine_error([&] { fmhost::option_formula_host(model, forward, forward_scalar, volatility, volatility_scalar, payoff_unit, payoff_unit_scalar, n, maturity, strike, outputs, out); });
}

void Engine::function_apply(fmhip_vec x, const int* kinds, int n_functions, fmhip_vec* out) {
    require_init();
    analytic_check_function(x, kinds, n_functions, out);
    pass_size(&x, 1, "named functions");
    pass_need_kernel(launch_function_apply != nullptr, "named-function");
    PassHold hold;
    pass_prepare(&x, 1, hold, "named functions");
    DevFunctionArgs a{};
    a.n = hold.n; a.n_functions = (uint32_t)n_functions;
    for (int f = 0; f < n_functions; ++f) a.kinds[f] = (uint32_t)kinds[f];
    a.x = hold.ptrs[0];
    PassOutputs outs(this);
    for (int f = 0; f < n_functions; ++f) a.out[f] = outs.add(hold.n);
    hip_check(launch_function_apply(a, stream_), "launch fm_function_apply_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (1 + n_functions);
    bytes_written_ += 4 * hold.n * n_functions;
    outs.commit(out);
}

void Engine::option_formula(int model, fmhip_vec forward, double forward_scalar, fmhip_vec volatility, double volatility_scalar, fmhip_vec payoff_unit,
                            double payoff_unit_scalar, double maturity, double strike, int outputs, fmhip_vec* out) {
    require_init();
    analytic_check_formula(model, forward, volatility, payoff_unit, maturity, strike, outputs, out);
    const fmhip_vec operands[3] = { forward, volatility, payoff_unit };
    fmhip_vec vectors[3]; int slot[3]; int n_vectors = 0;
    for (int k = 0; k < 3; ++k) if (operands[k]) { vectors[n_vectors] = operands[k]; slot[n_vectors++] = k; }
    pass_size(vectors, n_vectors, "option formula");
    pass_need_kernel(launch_option_formula != nullptr, "option-formula");
    PassHold hold;
    pass_prepare(vectors, n_vectors, hold, "option formula");
    const int n_out = fmhost::fm_formula_outputs(outputs);
    DevFormulaArgs a{};
    a.n = hold.n; a.model = (uint32_t)model; a.outputs = (uint32_t)outputs;
    a.scalar[0] = forward_scalar; a.scalar[1] = volatility_scalar; a.scalar[2] = payoff_unit_scalar;
    a.root_T = __builtin_sqrt(maturity); a.strike = strike;
    for (int v = 0; v < n_vectors; ++v) a.in[slot[v]] = hold.ptrs[(size_t)v];
    PassOutputs outs(this);
    for (int f = 0; f < n_out; ++f) a.out[f] = outs.add(hold.n);
    hip_check(launch_option_formula(a, stream_), "launch fm_option_formula_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_vectors + n_out);
    bytes_written_ += 4 * hold.n * n_out;
    outs.commit(out);
}

} // namespace fm
