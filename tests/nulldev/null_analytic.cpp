// null_analytic.cpp — TEST-ONLY stand-ins for the launchers of analytic_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  They refuse what the real launchers refuse (function_shape_ok, formula_shape_ok),
// read the last 16-byte group of every operand and write the last 16-byte group of every output the way the kernels do (a wild or
// undersized pointer is an ASan report), and — device memory being host memory here — compute the results THE KERNELS' WAY: group by group
// from the launch's own argument block (kinds, mask, output slots, operands that are a vector or a scalar), so that a wrong slot, scalar or
// address shows in what the driver compares with the definition.
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../finmath-lib-cuda-extensions_amd/csrc/analytic_kernel.h"

namespace fm {

hipError_t launch_function_apply(const DevFunctionArgs& a, hipStream_t) {
    if (!function_shape_ok(a)) return hipErrorInvalidValue;
    const float* x = reinterpret_cast<const float*>((uintptr_t)a.x);
    const int64_t groups = (a.n + 3) / 4;
    for (int64_t g = 0; g < groups; ++g)                                                       // whole groups: the capacity is a multiple of 256 bytes
        for (int j = 0; j < 4; ++j) {
            const float v = x[g * 4 + j];
            for (uint32_t f = 0; f < a.n_functions; ++f) reinterpret_cast<float*>((uintptr_t)a.out[f])[g * 4 + j] = fmhost::fm_function_value((int)a.kinds[f], v);
        }
    return hipSuccess;
}

hipError_t launch_option_formula(const DevFormulaArgs& a, hipStream_t) {
    if (!formula_shape_ok(a)) return hipErrorInvalidValue;
    const float* in[3];
    for (int k = 0; k < 3; ++k) in[k] = reinterpret_cast<const float*>((uintptr_t)a.in[k]);
    const int slot_delta = (int)(a.outputs & 1), slot_vega = slot_delta + (int)((a.outputs >> 1) & 1);
    const int64_t groups = (a.n + 3) / 4;
    for (int64_t g = 0; g < groups; ++g)
        for (int j = 0; j < 4; ++j) {
            const int64_t p = g * 4 + j;
            const fmhost::FmFormulaOut r = fmhost::fm_option_formula((int)a.model, in[0] ? (double)in[0][p] : a.scalar[0], in[1] ? (double)in[1][p] : a.scalar[1],
                                                                     in[2] ? (double)in[2][p] : a.scalar[2], a.root_T, a.strike);
            if (a.outputs & fmhost::FM_FORMULA_VALUE) reinterpret_cast<float*>((uintptr_t)a.out[0])[p] = fmhost::fm_narrow(r.value);
            if (a.outputs & fmhost::FM_FORMULA_DELTA) reinterpret_cast<float*>((uintptr_t)a.out[slot_delta])[p] = fmhost::fm_narrow(r.delta);
            if (a.outputs & fmhost::FM_FORMULA_VEGA) reinterpret_cast<float*>((uintptr_t)a.out[slot_vega])[p] = fmhost::fm_narrow(r.vega);
        }
    return hipSuccess;
}

} // namespace fm
