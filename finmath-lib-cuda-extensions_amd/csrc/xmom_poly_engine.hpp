// xmom_poly_engine.hpp — the engine's side of the polynomial regression in one pass (kernels: xmom_poly_kernel.hip;
// definition and argument checks: host/polynomial_regression.hpp).  Passes in the frame of side_pass_engine.hpp (which says what every such
// pass does), behind xmom_wide_engine.hpp: the first a reducing one, the second a producing one.
//
// xmom_poly_pass: the sums of fmhip_cross_moments_wide for the list [monomials of the states…, extra vectors…, dependents…] — from the STATES:
// the monomials are slots of the wide pass's list that carry exponents, and the kernel forms them in registers.  Laid out as xmom_wide_pass is.
// poly_eval: the fitted polynomial as a new vector: one launch, no wait (exponents and coefficients travel in the kernel arguments).
#include "runtime.hpp"
#include "xmom_poly_kernel.h"
#include "../host/polynomial_regression.hpp"

namespace fm {

static_assert(FM_POLY_MAX_STATES == fmhost::FM_POLY_MAX_STATES && FM_POLY_MAX_EXPONENT == fmhost::FM_POLY_MAX_EXPONENT && FM_POLY_MAX_EVAL == fmhost::FM_POLY_MAX_EVAL
              && FM_XMOMW_MAX == fmhost::FM_POLY_MAX_VECTORS, "xmom_poly_kernel.h and host/polynomial_regression.hpp describe the same passes");

// WEAK: see pass_need_kernel (tests/nulldev/null_xmom_poly.cpp has the stand-ins).
hipError_t launch_xmom_poly(const DevXmomPolyArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_poly_eval(const DevPolyEvalArgs& a, hipStream_t st) __attribute__((weak));

void poly_check_moments(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, const double* sums_out) {
    pass_as_engine_error([&] { fmhost::polynomialCheckMoments<fmhip_vec>(states, n_states, exponents, n_terms, extra_x, n_extra, y, n_y, sums_out); });
}
void poly_check_evaluate(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const double* coefficients, const fmhip_vec* out) {
    pass_as_engine_error([&] { fmhost::polynomialCheckEvaluate<fmhip_vec>(states, n_states, exponents, n_terms, extra_x, n_extra, coefficients, out); });
}
// fmhip_polynomial_cross_moments_host and fmhip_polynomial_evaluate_host: the definition, with its complaints as engine errors
void poly_cross_moments_host(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms, const float* const* extra_x, int n_extra, const float* const* y, int n_y, double* sums_out) {
    pass_as_engine_error([&] { fmhost::polynomialCrossMoments(states, n, n_states, exponents, n_terms, extra_x, n_extra, y, n_y, sums_out); });
}
void poly_evaluate_host(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms, const float* const* extra_x, int n_extra, const double* coefficients, float* out) {
    pass_as_engine_error([&] { fmhost::polynomialEvaluate(states, n, n_states, exponents, n_terms, extra_x, n_extra, coefficients, out); });
}

// states first, then the vectors among extra_x, then y: handles, one size, n > 0 — before anything is flushed or launched
static int poly_real(Engine& e, const fmhip_vec* states, int n_states, const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, fmhip_vec* real, const char* what) {
    int n_real = 0;
    for (int s = 0; s < n_states; ++s) real[n_real++] = states[s];
    for (int i = 0; i < n_extra; ++i) if (extra_x[i]) real[n_real++] = extra_x[i];
    for (int m = 0; m < n_y; ++m) real[n_real++] = y[m];
    e.pass_size(real, n_real, what);
    return n_real;
}

void Engine::xmom_poly_pass(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, double* sums_out) {
    require_init();
    poly_check_moments(states, n_states, exponents, n_terms, extra_x, n_extra, y, n_y, sums_out);
    fmhip_vec real[FM_POLY_MAX_STATES + FM_XMOMW_MAX];
    const int n_real = poly_real(*this, states, n_states, extra_x, n_extra, y, n_y, real, "polynomial cross moments");
    pass_need_kernel(launch_xmom_poly != nullptr, "polynomial cross-moments");
    PassHold hold;
    pass_prepare(real, n_real, hold, "polynomial cross moments");
    const int n_x = n_terms + n_extra, m = n_x + n_y;
    // pinned: [sums] [flag]
    const size_t out_bytes = pass_up256((size_t)FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES * 8);
    char* stage = (char*)ensure_stage(out_bytes + 64);
    DevXmomPolyArgs p{};
    DevXmomWideArgs& a = p.w;
    int r = 0;
    for (int s = 0; s < n_states; ++s) p.state[s] = hold.ptrs[(size_t)r++];
    p.n_states = (uint32_t)n_states;
    int slot = 0;
    for (int i = 0; i < n_terms; ++i) {
        const uint8_t* e = exponents + (size_t)i * n_states;
        for (int s = 0; s < n_states; ++s) p.max_exponent = std::max<uint32_t>(p.max_exponent, e[s]);
        a.vec[slot++] = xmom_poly_term_slot(e, n_states);
    }
    for (int i = 0; i < n_extra; ++i) a.vec[slot++] = extra_x[i] ? hold.ptrs[(size_t)r++] : FM_XMOMW_ONE;
    for (int k = 0; k < n_y; ++k) a.vec[slot++] = hold.ptrs[(size_t)r++];
    for (; slot < FM_XMOMW_MAX; ++slot) a.vec[slot] = FM_XMOMW_PAD;
    const uint32_t blocks = xmom_wide_blocks(hold.n);
    pass_scratch(256, (size_t)blocks * FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES * 8);
    double* out_host = reinterpret_cast<double*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + out_bytes);
    a.counter = (uint32_t*)pass_zero_;
    a.n = hold.n; a.chunks = (uint32_t)((hold.n + FM_XMOMW_CHUNK - 1) / FM_XMOMW_CHUNK);
    a.n_groups = (uint32_t)((m + FM_XMOMW_GROUP - 1) / FM_XMOMW_GROUP);
    a.partials = (double*)pass_other_;
    a.out_host = out_host;
    pass_launch(flag, a.done_flag, a.done_value, "polynomial cross-moments pass", [&] { return launch_xmom_poly(p, stream_); });
    double* o = sums_out;
    for (int i = 0; i < n_x; ++i) for (int j = i; j < n_x; ++j) *o++ = out_host[xmom_wide_entry(i, j)];
    for (int i = 0; i < n_x; ++i) for (int k = 0; k < n_y; ++k) *o++ = out_host[xmom_wide_entry(i, n_x + k)];
}

void Engine::poly_eval(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const double* coefficients, fmhip_vec* out) {
    require_init();
    poly_check_evaluate(states, n_states, exponents, n_terms, extra_x, n_extra, coefficients, out);
    fmhip_vec real[FM_POLY_MAX_STATES + FM_POLY_MAX_EVAL];
    const int n_real = poly_real(*this, states, n_states, extra_x, n_extra, nullptr, 0, real, "polynomial evaluation");
    pass_need_kernel(launch_poly_eval != nullptr, "polynomial evaluation");
    PassHold hold;
    pass_prepare(real, n_real, hold, "polynomial evaluation");
    DevPolyEvalArgs a{};
    int r = 0;
    for (int s = 0; s < n_states; ++s) a.state[s] = hold.ptrs[(size_t)r++];
    for (int i = 0; i < n_terms; ++i) {
        uint32_t e = 0;
        for (int s = 0; s < n_states; ++s) e |= (uint32_t)exponents[(size_t)i * n_states + s] << (3 * s);
        a.exponents[i] = e;
    }
    for (int i = 0; i < n_extra; ++i) a.extra[i] = extra_x[i] ? hold.ptrs[(size_t)r++] : 0;
    for (int i = 0; i < n_terms + n_extra; ++i) a.coefficient[i] = (float)coefficients[i];
    a.n = hold.n; a.n_states = (uint32_t)n_states; a.n_terms = (uint32_t)n_terms; a.n_extra = (uint32_t)n_extra;
    PassOutputs outs(this);
    a.out = outs.add(hold.n);
    hip_check(launch_poly_eval(a, stream_), "launch fm_poly_eval_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_real + 1);
    bytes_written_ += 4 * hold.n;
    outs.commit(out);
}

} // namespace fm
