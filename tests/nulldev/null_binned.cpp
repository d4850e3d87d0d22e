// null_binned.cpp — TEST-ONLY stand-ins for the two launchers of binned_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  They refuse what the real launchers refuse (binned_*_shape_ok), touch the first
// and last element of every scratch array the launch is handed (a wild or undersized pointer is an ASan report), and — device memory being
// host memory here — compute the counts, the sums and the estimate with the host definition (host/binned_regression.hpp), entry by entry in
// the layout the engine asked for, so that the driver can check what comes back; the completion flag is raised.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/binned_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/binned_regression.hpp"

namespace fm {

hipError_t launch_binned_xmom(const DevBinnedXmomArgs& a, hipStream_t) {
    if (!binned_xmom_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t blocks = binned_blocks(a.n);
    for (int k = 0; k <= FM_BINNED_MAX_SLICES; ++k) if (((volatile uint32_t*)a.counters)[k] != 0u) return hipErrorInvalidValue;      // zero between launches
    for (int k = 0; k < FM_BINNED_MAX_BINS; ++k) if (((volatile uint32_t*)a.counts_dev)[k] != 0u) return hipErrorInvalidValue;
    a.partials[0] = 0.0;
    a.partials[(size_t)a.n_slices * FM_BINNED_ENTRIES * blocks - 1] = 0.0;
    const float* key = reinterpret_cast<const float*>((uintptr_t)a.key);
    const float* x[FM_BINNED_MAX_X]; const float* y[FM_BINNED_MAX_Y];
    for (uint32_t i = 0; i < a.n_x; ++i) x[i] = reinterpret_cast<const float*>((uintptr_t)a.x[i]);
    for (uint32_t m = 0; m < a.n_y; ++m) y[m] = reinterpret_cast<const float*>((uintptr_t)a.y[m]);
    const int q = fmhost::binnedSumsPerBin((int)a.n_x, (int)a.n_y);
    std::vector<int64_t> counts(a.n_bins);
    std::vector<double> sums((size_t)a.n_bins * q);
    try { fmhost::binnedCrossMoments(key, a.n, a.bounds, (int)a.n_bins, x, (int)a.n_x, a.n_y ? y : nullptr, (int)a.n_y, counts.data(), sums.data()); }
    catch (const std::invalid_argument&) { return hipErrorInvalidValue; }
    for (uint32_t b = 0; b < a.n_bins; ++b) {
        a.counts_host[b] = (uint32_t)counts[b];
        int at = 0;                                             // the definition's packed layout -> the slots of the full shape -> the entries
        for (uint32_t i = 0; i < a.n_x; ++i) for (uint32_t c = i; c < a.n_x; ++c, ++at) {
            const int e = a.slot_entry[i * FM_BINNED_MAX_X - i * (i - 1) / 2 + (c - i)];
            if (e >= 0) a.out_host[(size_t)b * a.entries_per_bin + e] = sums[(size_t)b * q + at];
        }
        for (uint32_t i = 0; i < a.n_x; ++i) for (uint32_t m = 0; m < a.n_y; ++m, ++at) {
            const int e = a.slot_entry[FM_BINNED_MAX_X * (FM_BINNED_MAX_X + 1) / 2 + i * FM_BINNED_MAX_Y + m];
            if (e >= 0) a.out_host[(size_t)b * a.entries_per_bin + e] = sums[(size_t)b * q + at];
        }
    }
    __atomic_store_n(a.done_flag, a.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

hipError_t launch_binned_eval(const DevBinnedEvalArgs& a, hipStream_t) {
    if (!binned_eval_shape_ok(a)) return hipErrorInvalidValue;
    const float* key = reinterpret_cast<const float*>((uintptr_t)a.key);
    float* out = reinterpret_cast<float*>((uintptr_t)a.out);
    const float* x[FM_BINNED_MAX_X];
    for (uint32_t i = 0; i < a.n_x; ++i) x[i] = reinterpret_cast<const float*>((uintptr_t)a.x[i]);
    std::vector<double> c((size_t)a.n_bins * a.n_x);
    for (size_t i = 0; i < c.size(); ++i) c[i] = (double)a.coefficients[i];
    try { fmhost::binnedEvaluate(key, a.n, a.bounds, (int)a.n_bins, x, (int)a.n_x, c.data(), out); }
    catch (const std::invalid_argument&) { return hipErrorInvalidValue; }
    return hipSuccess;
}

} // namespace fm
