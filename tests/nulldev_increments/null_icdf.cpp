// null_icdf.cpp — TEST-ONLY stand-in for the launcher of fm_mt_icdf_kernel (mt_bm_kernel.hip), beside the null device of tests/nulldev and
// the stand-in for the jump launcher (tests/nulldev_mersenne/null_mt.cpp).  Device memory being host memory here, it does what the kernel
// does the plain way: from the STATE, the DESCRIPTORS and the TABLES the engine hands it — nothing is rebuilt from the caller's laws — it
// draws one uniform after the other (host/mersenne.hpp) and applies the descriptor of the stream as the kernel does: the normal law by
// inverseNormalCdf, the uniform law by a + (b − a)·u, the Poisson law by comparing with the table it is pointed to.  So the driver can check
// against fmhip_increments_host that the engine seeds, jumps, shares tables between equal means, and lays descriptors, tables and the slab
// out as the kernel expects; a wild or undersized pointer is an ASan report.
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/mt_bm_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/mersenne.hpp"

namespace fm {

std::atomic<int> g_null_icdf_tables{ 0 }, g_null_icdf_table_doubles{ 0 };     // what the last launch was handed: distinct tables, their doubles (the driver reads these; shards launch side by side)

hipError_t launch_mt_icdf(const DevMtIcdfArgs& A, hipStream_t) {
    const DevMtBmArgs& a = A.g;
    if (a.n_paths <= 0) return hipSuccess;
    if (!a.slab || !A.laws || !A.tables || !a.state || a.sqrt_dt || a.n_streams == 0 || a.stride_floats < a.n_paths || (a.stride_floats & 63)) return hipErrorInvalidValue;
    if (a.segment_log2 < (uint32_t)FM_MT_MIN_SEGMENT_LOG2 || a.segment_log2 > (uint32_t)FM_MT_MAX_SEGMENT_LOG2) return hipErrorInvalidValue;
    const uint64_t words = 2ull * a.n_streams * (uint64_t)a.n_paths;
    if (a.n_segments != (uint32_t)((words + (1ull << a.segment_log2) - 1) >> a.segment_log2)) return hipErrorInvalidValue;
    if (a.tile_paths && ((a.tile_paths & 3u) || (uint64_t)a.tile_paths * a.n_streams > (uint64_t)FM_MT_TILE_FLOATS || (uint64_t)a.tile_paths * a.n_streams < 256u)) return hipErrorInvalidValue;
    if (((uintptr_t)A.laws & 15u) || ((uintptr_t)A.tables & 7u) || ((uintptr_t)a.state & 3u)) return hipErrorInvalidValue;
    // the tables: one behind the other without gaps, each rising and ending in 1.0
    uint32_t end = 0; int tables = 0;
    for (uint32_t s = 0; s < a.n_streams; ++s) {
        const DevMtLaw& L = A.laws[s];
        if (L.kind < 0 || L.kind > 2) return hipErrorInvalidValue;
        if (L.kind != 2) { if (L.table_len || L.table_offset) return hipErrorInvalidValue; continue; }
        if (L.table_len == 0 || L.table_offset > end) return hipErrorInvalidValue;             // a table starts where an earlier one ended, or is an earlier one
        if (L.table_offset == end) { end += L.table_len; ++tables; }
        else if (L.table_offset + L.table_len > end) return hipErrorInvalidValue;
        const double* F = A.tables + L.table_offset;
        for (uint32_t k = 1; k < L.table_len; ++k) if (!(F[k] >= F[k - 1])) return hipErrorInvalidValue;
        if (F[L.table_len - 1] != 1.0) return hipErrorInvalidValue;
    }
    g_null_icdf_tables = tables; g_null_icdf_table_doubles = (int)end;
    fmhost::MT19937 mt((int64_t)0);
    std::memcpy(mt.mt, a.state, sizeof mt.mt);
    mt.mti = 624;
    for (int64_t p = 0; p < a.n_paths; ++p)
        for (uint32_t s = 0; s < a.n_streams; ++s) {
            const DevMtLaw& L = A.laws[s];
            const double u = mt.nextDouble();
            double v;
            if (L.kind == 0) v = fmhost::inverseNormalCdf(u) * L.a;
            else if (L.kind == 1) { const double width = L.b - L.a; const double scaled = width * u; v = L.a + scaled; }
            else {
                const double* F = A.tables + L.table_offset;
                uint32_t k = 0;
                while (k + 1 < L.table_len && F[k] < u) ++k;
                v = (double)k;
            }
            a.slab[(size_t)s * a.stride_floats + p] = (float)v;
        }
    return hipSuccess;
}

} // namespace fm
