// analytic_double_shim.cpp — the fp64 functions of host/normal_functions.hpp behind a C interface, for tests/test_analytic_cpu.py: the
// library's entry points narrow to fp32, and the accuracy condition of DESIGN.md §4.21 is about the doubles.  Built by the test with the
// library's flags (-ffp-contract=off), loaded through ctypes.  Not part of the library.
#include "../../finmath-lib-cuda-extensions_amd/host/normal_functions.hpp"

extern "C" {

void shim_function64(int kind, const double* x, int64_t n, double* out)
{
    for (int64_t p = 0; p < n; ++p)
        out[p] = kind == fmhost::FM_FN_NORMAL_CDF ? fmhost::fm_normal_cdf(x[p]) : kind == fmhost::FM_FN_NORMAL_DENSITY ? fmhost::fm_normal_density(x[p]) : fmhost::fm_normal_quantile_checked(x[p]);
}

// out[p][0..3): value, delta, vega
void shim_formula64(int model, const double* forward, const double* volatility, const double* payoff_unit, int64_t n, double maturity, double strike, double* out)
{
    const double root_T = __builtin_sqrt(maturity);
    for (int64_t p = 0; p < n; ++p) {
        const fmhost::FmFormulaOut r = fmhost::fm_option_formula(model, forward[p], volatility[p], payoff_unit[p], root_T, strike);
        out[3 * p] = r.value; out[3 * p + 1] = r.delta; out[3 * p + 2] = r.vega;
    }
}

} // extern "C"
