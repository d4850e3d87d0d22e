// null_table.cpp — TEST-ONLY stand-in for the launcher of table_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp: device
// memory is host memory, launches compute nothing).  It refuses what the real launcher refuses (table_shape_ok), touches the first and last
// element of every table the launch is handed and the last 16-byte group of every output the way the kernel does (a wild or undersized
// pointer is an ASan report), and — device memory being host memory here — computes the results THE KERNEL'S WAY: the segment by the index
// that the engine built (fm_table_segment), so that a wrong index, scale or layout shows in what the driver compares with the definition.
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../finmath-lib-cuda-extensions_amd/csrc/table_kernel.h"

namespace fm {

hipError_t launch_table_apply(const DevTableArgs& a, hipStream_t) {
    if (!table_shape_ok(a)) return hipErrorInvalidValue;
    const int m = (int)a.m, T = (int)a.n_tables, cells = (int)a.cells;
    if (a.first[0] != 0 || a.first[cells] != (uint16_t)(m - 1)) return hipErrorInvalidValue;      // every knot but the last has a cell
    for (int c = 0; c < cells; ++c) if (a.first[c] > a.first[c + 1]) return hipErrorInvalidValue;
    const float* x = reinterpret_cast<const float*>((uintptr_t)a.x);
    const int64_t groups = (a.n + 3) / 4;
    for (int f = 0; f < T; ++f) {
        float* out = reinterpret_cast<float*>((uintptr_t)a.out[f]);
        for (int j = 0; j < 4; ++j) out[(groups - 1) * 4 + j] = 0.0f;                            // whole groups: the capacity is a multiple of 256 bytes
    }
    volatile float past = 0.0f;
    for (int j = 0; j < 4; ++j) past = past + x[(groups - 1) * 4 + j] * 0.0f;
    for (int64_t p = 0; p < a.n; ++p) {
        const double X = (double)x[p];
        const int s = fmhost::fm_table_segment(a.knots, m, a.first, cells, a.scale, X);
        const double anchor = a.knots[s > 0 ? s - 1 : 0];
        for (int f = 0; f < T; ++f)
            reinterpret_cast<float*>((uintptr_t)a.out[f])[p] = fmhost::fm_table_value(a.coefficients + ((size_t)f * (size_t)(m + 1) + (size_t)s) * 4, X, anchor);
    }
    return hipSuccess;
}

} // namespace fm
