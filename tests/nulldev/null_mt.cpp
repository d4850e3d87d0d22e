// null_mt.cpp — TEST-ONLY stand-ins for the three launchers of mt_bm_kernel.hip, beside the null device (null_hip.cpp: device memory is host
// memory, launches compute nothing).  Device memory being host memory here, the stand-ins do what the kernels do the plain way: the jump
// with host/mt_jump.hpp, the increments one after the other with host/mersenne.hpp from the STATE they are handed — and, for
// fm_mt_icdf_kernel, from the DESCRIPTORS and the TABLES they are handed: nothing is rebuilt from the caller's laws; the normal law by
// inverseNormalCdf, the uniform law by a + (b − a)·u, the Poisson law by comparing with the table it is pointed to.  So the drivers can
// check against fmhip_mersenne_increments and fmhip_increments_host that the engine seeds, jumps (path offsets, shards), shares tables
// between equal means and lays descriptors, tables and the slab out as the kernels expect (the launchers' own check, mt_shape_ok, is
// applied to the arguments), and a wild or undersized pointer is an ASan report.
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/mt_bm_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/mt_jump.hpp"

namespace fm {

std::atomic<int> g_null_icdf_tables{ 0 }, g_null_icdf_table_doubles{ 0 };     // what the last launch was handed: distinct tables, their doubles (the driver reads these; shards launch side by side)

hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t) {
    if (!in || !out || in == out) return hipErrorInvalidValue;
    std::memcpy(out, in, sizeof(uint32_t) * FM_MT_STATE_WORDS);
    try { fmhost::mtJump(out, distance); } catch (...) { return hipErrorInvalidValue; }
    return hipSuccess;
}

// path after path, stream after stream from the handed state: draw(stream, uniform) is the increment in fp64
template <class Draw>
static void generate(const DevMtBmArgs& a, Draw draw) {
    fmhost::MT19937 mt((int64_t)0);
    std::memcpy(mt.mt, a.state, sizeof mt.mt);
    mt.mti = 624;
    for (int64_t p = 0; p < a.n_paths; ++p)
        for (uint32_t s = 0; s < a.n_streams; ++s)
            a.slab[(size_t)s * a.stride_floats + p] = (float)draw(s, mt.nextDouble());
}

hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t) {
    if (a.n_paths <= 0) return hipSuccess;
    if (!mt_shape_ok(a)) return hipErrorInvalidValue;
    generate(a, [&](uint32_t s, double u) { return fmhost::inverseNormalCdf(u) * a.sqrt_dt[s]; });
    return hipSuccess;
}

hipError_t launch_mt_icdf(const DevMtIcdfArgs& A, hipStream_t) {
    const DevMtBmArgs& a = A.g;
    if (a.n_paths <= 0) return hipSuccess;
    if (!mt_shape_ok(a, &A)) return hipErrorInvalidValue;
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
    generate(a, [&](uint32_t s, double u) {
        const DevMtLaw& L = A.laws[s];
        if (L.kind == 0) return fmhost::inverseNormalCdf(u) * L.a;
        if (L.kind == 1) { const double width = L.b - L.a; const double scaled = width * u; return L.a + scaled; }
        const double* F = A.tables + L.table_offset;
        uint32_t k = 0;
        while (k + 1 < L.table_len && F[k] < u) ++k;
        return (double)k;
    });
    return hipSuccess;
}

} // namespace fm
