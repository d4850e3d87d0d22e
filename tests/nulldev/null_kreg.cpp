// null_kreg.cpp — TEST-ONLY stand-in for the launcher of kreg_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp: device
// memory is host memory, launches compute nothing).  It refuses what the real launcher refuses (kernel_moments_shape_ok), checks that the
// counters are zero between launches and that the tables the engine sent up are the ones the definition makes of points and bandwidths,
// touches the first and last element of every scratch array the launch is handed (a wild or undersized pointer is an ASan report), and —
// device memory being host memory here — computes the sums with the host definition (host/kernel_regression.hpp) from the tables, slice by
// slice in the layout the engine asked for, so that the driver can check what comes back; the completion flag is raised.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/kreg_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/kernel_regression.hpp"

namespace fm {

hipError_t launch_kernel_moments(const DevKernelMomentsArgs& a, hipStream_t) {
    if (!kernel_moments_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t blocks = binned_blocks(a.n), Q = a.n_points, qe = a.entries_per_point;
    for (int k = 0; k <= FM_KREG_MAX_SLICES; ++k) if (((volatile uint32_t*)a.counters)[k] != 0u) return hipErrorInvalidValue;      // zero between launches
    a.partials[0] = 0.0;
    a.partials[(size_t)a.n_slices * FM_KREG_ENTRIES * blocks - 1] = 0.0;
    const double* lower = a.tables; const double* upper = a.tables + Q; const double* points = a.tables + 2 * (size_t)Q; const double* rh = a.tables + 3 * (size_t)Q;
    std::vector<double> h(Q);
    for (uint32_t q = 0; q < Q; ++q) {
        h[q] = (upper[q] - lower[q]) * 0.5;                    // the drivers' grids are dyadic: exact
        if (lower[q] != points[q] - h[q] || upper[q] != points[q] + h[q] || rh[q] != 1.0 / h[q]) return hipErrorInvalidValue;
    }
    const float* key = reinterpret_cast<const float*>((uintptr_t)a.key);
    const float* y[FM_KREG_MAX_Y] = {};
    for (uint32_t m = 0; m < a.n_y; ++m) y[m] = reinterpret_cast<const float*>((uintptr_t)a.y[m]);
    const int64_t groups = (a.n + 3) / 4;                      // whole 16-byte groups are read: the capacity is a multiple of 256 bytes
    volatile float past = 0.0f;
    for (int j = 0; j < 4; ++j) { past = past + key[(groups - 1) * 4 + j] * 0.0f; for (uint32_t m = 0; m < a.n_y; ++m) past = past + y[m][(groups - 1) * 4 + j] * 0.0f; }
    // slice by slice, as the grid's y does: the points of a slice and nothing else
    for (uint32_t s = 0; s < a.n_slices; ++s) {
        const uint32_t lo = s * a.points_per_slice, np = Q - lo < a.points_per_slice ? Q - lo : a.points_per_slice;
        std::vector<double> sums((size_t)np * qe);
        try { fmhost::kernel_moments_host(key, a.n, points + lo, h.data() + lo, (int)np, (int)a.kernel, (int)a.order, a.n_y ? y : nullptr, (int)a.n_y, sums.data()); }
        catch (const std::invalid_argument&) { return hipErrorInvalidValue; }
        for (size_t e = 0; e < sums.size(); ++e) a.out_host[(size_t)lo * qe + e] = sums[e];
    }
    __atomic_store_n(a.done_flag, a.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

} // namespace fm
