// null_xmom.cpp — TEST-ONLY stand-in for the cross-moments launcher of kernels.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  The first and last element of every vector and of the scratch arrays the launch
// is handed are touched (a wild or undersized pointer is an ASan report), and — device memory being host memory here — the sums are
// computed the plain way, product by product in fp64, so the driver can check the layout of what comes back; the completion flag is raised.
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../finmath-lib-cuda-extensions_amd/csrc/kernels.h"

namespace fm {

hipError_t launch_xmom(const DevXmomArgs& a, hipStream_t) {
    if (a.n <= 0 || a.n_blocks == 0 || a.n_blocks > (uint32_t)FM_XMOM_MAX_BLOCKS) return hipErrorInvalidValue;
    const uint32_t blocks = xmom_blocks(a.n);
    for (uint32_t k = 0; k <= (uint32_t)FM_XMOM_MAX_BLOCKS; ++k) if (((volatile uint32_t*)a.counters)[k] != 0u) return hipErrorInvalidValue;      // zero between launches
    for (uint32_t b = 0; b < a.n_blocks; ++b) {
        a.partials[(size_t)b * FM_XMOM_PAIRS * blocks] = 0.0;
        a.partials[(size_t)(b + 1) * FM_XMOM_PAIRS * blocks - 1] = 0.0;
        for (int r = 0; r < FM_XMOM_GROUP; ++r)
            for (int c = 0; c < FM_XMOM_GROUP; ++c) {
                const float* x = reinterpret_cast<const float*>((uintptr_t)a.vec[a.row_group[b] * FM_XMOM_GROUP + r]);
                const float* y = reinterpret_cast<const float*>((uintptr_t)a.vec[a.col_group[b] * FM_XMOM_GROUP + c]);
                double s = 0.0;
                for (int64_t p = 0; p < a.n; ++p) s += (x ? (double)x[p] : 1.0) * (y ? (double)y[p] : 1.0);
                a.out_host[(size_t)b * FM_XMOM_PAIRS + (size_t)r * FM_XMOM_GROUP + c] = s;
            }
    }
    __atomic_store_n(a.done_flag, a.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

} // namespace fm
