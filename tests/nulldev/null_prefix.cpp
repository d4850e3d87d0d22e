// null_prefix.cpp — TEST-ONLY stand-ins for the two launchers of prefix_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real work the
// plain way, phase by phase as the kernels do: every chunk of prefix_chunk_tiles / prefix_blocks is scanned on its own (prefix_unit_host
// at the chunk's level) and leaves its row { total, largest prefix inside } exactly where the totals kernel writes it; the carry is the
// serial chain over the rows, written where the carry kernel writes it, and locates every query's chunk; apply and query add the chunk's
// base.  So the engine's scratch is used at its full size — rows[blocks − 1], bases[blocks], queries[count − 1], located[count − 1] — and
// the padded quads that the 16-byte loads and stores reach are touched (an undersized scratch or buffer is an ASan report).  The flag is
// raised by launch_sort_done (null_sort.cpp).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/prefix_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
uint32_t last_of_quads(uint32_t n) { return ((n + 3u) & ~3u) - 1u; }      // storage is padded to 256 bytes: the kernels read and write whole quads

// totals and carry; local[r]: the prefix of r inside its chunk
struct Phases {
    std::vector<double> local;
    uint32_t blocks; int64_t chunk;
    Phases(const DevPrefixArgs& a) : local(a.n), blocks(prefix_blocks((int64_t)a.n)), chunk(prefix_chunk_elems((int64_t)a.n))
    {
        const float* v = at<const float>(a.v);
        (void)*(volatile const float*)&v[last_of_quads(a.n)];
        PrefixRow* rows = prefix_rows(a);
        double* bases = prefix_bases(a);
        for (uint32_t c = 0; c < blocks; ++c) {
            const int64_t e0 = (int64_t)c * chunk, cnt = std::min<int64_t>(chunk, (int64_t)a.n - e0);
            prefix_unit_host(v + e0, cnt, local.data() + e0, 5, chunk);
            double largest = std::numeric_limits<double>::quiet_NaN();
            for (int64_t i = 0; i < cnt; ++i) { const double x = local[(size_t)(e0 + i)]; if (x > largest || largest != largest) largest = x; }
            rows[c] = PrefixRow{ local[(size_t)(e0 + cnt - 1)], largest };
        }
        double run = rows[0].total;
        bases[0] = 0.0;
        for (uint32_t c = 1; c < blocks; ++c) { bases[c] = run; run = run + rows[c].total; }
        bases[blocks] = run;
        if (a.total_host) *a.total_host = run;
    }
    double P(const DevPrefixArgs& a, int64_t r) const { const int64_t c = r / chunk; return c == 0 ? local[(size_t)r] : prefix_bases(a)[c] + local[(size_t)r]; }
};
}

hipError_t launch_prefix_sums(const DevPrefixArgs& a, hipStream_t) {
    if (!prefix_shape_ok(a) || a.kind != FM_PREFIX_QUERY_NONE) return hipErrorInvalidValue;
    const Phases ph(a);
    float* out = at<float>(a.out);
    out[last_of_quads(a.n)] = 0.f;
    for (int64_t r = 0; r < (int64_t)a.n; ++r) out[r] = prefix_out_host(ph.P(a, r), r, (int)a.mode);
    return hipSuccess;
}

hipError_t launch_prefix_queries(const DevPrefixArgs& a, hipStream_t) {
    if (!prefix_shape_ok(a) || a.kind == FM_PREFIX_QUERY_NONE) return hipErrorInvalidValue;
    const Phases ph(a);
    const uint64_t* queries = prefix_queries(a);
    PrefixLocated* located = prefix_located(a);
    const PrefixRow* rows = prefix_rows(a);
    const double* bases = prefix_bases(a);
    const int64_t n = (int64_t)a.n;
    for (uint32_t j = 0; j < a.count; ++j) {
        if (a.kind == FM_PREFIX_QUERY_AT) {
            const uint64_t pos = queries[j];
            if (pos >= (uint64_t)n) return hipErrorInvalidValue;
            located[j] = PrefixLocated{ 0.0, (uint32_t)((int64_t)pos / ph.chunk), 0u };
            a.sums_host[j] = ph.P(a, (int64_t)pos);
            continue;
        }
        double t; std::memcpy(&t, &queries[j], 8);
        if (a.relative) t = t * bases[ph.blocks];
        uint32_t c = 0;
        for (; c < ph.blocks; ++c) { const double top = c == 0 ? rows[0].largest : bases[c] + rows[c].largest; if (top >= t) break; }
        located[j] = PrefixLocated{ t, c, 0u };
        int64_t hit = n;
        if (c < ph.blocks) {
            const int64_t e0 = (int64_t)c * ph.chunk, e1 = std::min<int64_t>(e0 + ph.chunk, n);
            for (int64_t r = e0; r < e1; ++r) if (ph.P(a, r) >= t) { hit = r; break; }
            if (hit == n) return hipErrorInvalidValue;             // a located chunk holds its crossing
        }
        a.positions_host[j] = (uint64_t)hit;
        a.sums_host[j] = hit < n ? ph.P(a, hit) : bases[ph.blocks];
    }
    return hipSuccess;
}

} // namespace fm
