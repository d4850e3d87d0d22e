// transform_double_shim.cpp — the fp64 results of host/trig64.hpp and host/transform_formula.hpp behind a C interface, for
// tests/test_transform_formula_cpu.py: the library's entry points narrow to fp32, and the accuracy conditions of DESIGN.md §4.28 are about
// the doubles.  Built by the test with the library's flags (-ffp-contract=off) by g++ and by hipcc -x c++, loaded through ctypes.  Not part
// of the library.
#include "../../finmath-lib-cuda-extensions_amd/host/transform_formula.hpp"

extern "C" {

double shim_trig_max() { return fmhost::FM_TRIG_MAX; }
double shim_trig_error_ulps() { return fmhost::FM_TRIG_ERROR_ULPS; }

void shim_sincos64(const double* theta, int64_t n, double* sine, double* cosine)
{
    for (int64_t p = 0; p < n; ++p) {
        const fmhost::FmSinCos r = fmhost::fm_sincos64(theta[p]);
        sine[p] = r.sin; cosine[p] = r.cos;
    }
}

// out[p][0..3): value, delta, state delta, before they are narrowed
void shim_transform64(const double* nodes, int n_nodes, int n_states, const double* forward, const double* payoff_unit, const double* state0, const double* state1, int64_t n,
                      double strike, double* out)
{
    for (int64_t p = 0; p < n; ++p) {
        const fmhost::FmTransformOut r = fmhost::fm_transform_option(nodes, n_nodes, n_states, forward[p], payoff_unit[p], state0[p], state1[p], strike);
        out[3 * p] = r.value; out[3 * p + 1] = r.delta; out[3 * p + 2] = r.state_delta;
    }
}

} // extern "C"
