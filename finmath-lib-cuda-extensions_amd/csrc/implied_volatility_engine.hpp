// implied_volatility_engine.hpp — the engine's side of the implied volatility per path (kernel:
// implied_volatility_kernel.hip; definition and argument check: host/implied_volatility.hpp).  A producing pass in the frame of
// side_pass_engine.hpp (which says what every such pass does), beside the option formulas of analytic_engine.hpp, whose inverse it is.
//
// implied_volatility: the volatility (and, by a mask, its partials in the price and in the forward) at which a Black–Scholes or Bachelier
// call whose price, forward and payoff unit are each a vector or a scalar has that price; one new vector per set bit.  One launch, not
// waited for; nothing goes through the pinned stage — the arguments are the launch's.  The pass is elementwise: a device list runs it per
// shard (sharded.cpp), a communicator's ranks each on their own paths.
#include "runtime.hpp"
#include "implied_volatility_kernel.h"

namespace fm {

static_assert(FMHIP_IMPLIED_VOLATILITY == fmhost::FM_IMPLIED_VOLATILITY && FMHIP_IMPLIED_D_PRICE == fmhost::FM_IMPLIED_D_PRICE
              && FMHIP_IMPLIED_D_FORWARD == fmhost::FM_IMPLIED_D_FORWARD,
              "include/fmhip.h and host/implied_volatility.hpp name the same outputs");

// WEAK: see pass_need_kernel (tests/nulldev/null_implied_volatility.cpp has the stand-in).
hipError_t launch_implied_volatility(const DevImpliedArgs& a, hipStream_t st) __attribute__((weak));

void implied_check(int model, fmhip_vec price, fmhip_vec forward, fmhip_vec payoff_unit, double maturity, double strike, int outputs, const fmhip_vec* out) {
    pass_as_engine_error([&] { fmhost::impliedCheck(model, maturity, strike, outputs, out); });
    if (!price && !forward && !payoff_unit) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "implied volatility: at least one of price, forward and payoff unit is a vector");
}
// fmhip_implied_volatility_host: the definition, with its complaints as engine errors
void implied_volatility_host_checked(int model, const float* price, double price_scalar, const float* forward, double forward_scalar, const float* payoff_unit,
                                     double payoff_unit_scalar, int64_t n, double maturity, double strike, int outputs, float* const* out) {
    pass_as_engine_error([&] { fmhost::implied_volatility_host(model, price, price_scalar, forward, forward_scalar, payoff_unit, payoff_unit_scalar, n, maturity, strike, outputs, out); });
}

void Engine::implied_volatility(int model, fmhip_vec price, double price_scalar, fmhip_vec forward, double forward_scalar, fmhip_vec payoff_unit,
                                double payoff_unit_scalar, double maturity, double strike, int outputs, fmhip_vec* out) {
    require_init();
    implied_check(model, price, forward, payoff_unit, maturity, strike, outputs, out);
    const fmhip_vec operands[3] = { price, forward, payoff_unit };
    fmhip_vec vectors[3]; int slot[3]; int n_vectors = 0;
    for (int k = 0; k < 3; ++k) if (operands[k]) { vectors[n_vectors] = operands[k]; slot[n_vectors++] = k; }
    pass_size(vectors, n_vectors, "implied volatility");
    pass_need_kernel(launch_implied_volatility != nullptr, "implied-volatility");
    PassHold hold;
    pass_prepare(vectors, n_vectors, hold, "implied volatility");
    const int n_out = fmhost::fm_formula_outputs(outputs);
    DevImpliedArgs a{};
    a.n = hold.n; a.model = (uint32_t)model; a.outputs = (uint32_t)outputs;
    a.scalar[0] = price_scalar; a.scalar[1] = forward_scalar; a.scalar[2] = payoff_unit_scalar;
    a.root_T = __builtin_sqrt(maturity); a.strike = strike;
    for (int v = 0; v < n_vectors; ++v) a.in[slot[v]] = hold.ptrs[(size_t)v];
    PassOutputs outs(this);
    for (int f = 0; f < n_out; ++f) a.out[f] = outs.add(hold.n);
    hip_check(launch_implied_volatility(a, stream_), "launch fm_implied_volatility_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_vectors + n_out);
    bytes_written_ += 4 * hold.n * n_out;
    outs.commit(out);
}

} // namespace fm
