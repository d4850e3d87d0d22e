// null_resample.cpp — TEST-ONLY stand-in for the launcher of resample_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-in does the real work phase
// by phase as the kernels do: every chunk of the CLEANED weights is scanned on its own (prefix_unit_host at the chunk's level) and leaves
// its total where the totals kernel writes it; the carry is the serial chain over the totals, written where the carry kernel writes it;
// P goes into the temporary at its full size; the gather walks its tiles of FM_RESAMPLE_TILE outputs the kernel's way — the table of the
// chunks' last prefixes, a bisection of it and one inside the chunk with the kernel's trip counts (resample_search of resample_host.hpp), the
// clamp, the loads, the stores.  So the scratch, the temporary and the padded quads that the 16-byte loads reach are touched (an undersized
// buffer is an ASan report).  The flag is raised by launch_sort_done (null_sort.cpp).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/resample_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
uint32_t last_of_quads(uint32_t n) { return ((n + 3u) & ~3u) - 1u; }      // storage is padded to 256 bytes: the prefix kernels read whole quads
}

hipError_t launch_resample(const DevResampleArgs& a, hipStream_t) {
    if (!resample_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)a.n, m = (int64_t)a.m;
    const uint32_t blocks = prefix_blocks(n);
    const int64_t chunk = prefix_chunk_elems(n);
    double total = (double)n;
    std::vector<double> tops;
    if (a.weights) {
        const float* w = at<const float>(a.weights);
        (void)*(volatile const float*)&w[last_of_quads(a.n)];
        std::vector<float> cw((size_t)n);
        for (int64_t r = 0; r < n; ++r) cw[(size_t)r] = resample_clean(w[r]);
        double* totals = resample_totals(a);
        double* bases = resample_bases(a);
        double* P = a.prefix;
        // totals: every chunk on its own, its prefixes inside the chunk parked in P
        for (uint32_t c = 0; c < blocks; ++c) {
            const int64_t e0 = (int64_t)c * chunk, cnt = std::min<int64_t>(chunk, n - e0);
            prefix_unit_host(cw.data() + e0, cnt, P + e0, 5, chunk);
            totals[c] = P[e0 + cnt - 1];
        }
        // carry
        double run = totals[0];
        bases[0] = 0.0;
        for (uint32_t c = 1; c < blocks; ++c) { bases[c] = run; run = run + totals[c]; }
        bases[blocks] = run;
        if (a.total_host) *a.total_host = run;
        // prefixes
        for (uint32_t c = 1; c < blocks; ++c) {
            const int64_t e0 = (int64_t)c * chunk, e1 = std::min<int64_t>(e0 + chunk, n);
            for (int64_t r = e0; r < e1; ++r) P[r] = bases[c] + P[r];
        }
        tops.assign(bases + 1, bases + 1 + blocks);
        total = bases[blocks];
    }
    // gather, tile by tile
    const bool degenerate = resample_degenerate(total);
    const int chunk_trips = resample_trips((int64_t)blocks), inner_trips = resample_trips(std::min(chunk, n));
    const float* uniforms = at<const float>(a.uniforms);
    uint32_t* ancestors = at<uint32_t>(a.ancestors_out);
    for (int64_t tile = 0; tile * FM_RESAMPLE_TILE < m; ++tile) {
        for (int64_t j = tile * FM_RESAMPLE_TILE; j < std::min<int64_t>((tile + 1) * FM_RESAMPLE_TILE, m); ++j) {
            double U = 0.0;
            bool alive = !degenerate;
            if (alive && resample_needs_uniforms((int)a.scheme)) alive = resample_uniform(uniforms[j], U);
            const double t = alive ? resample_target(resample_fraction((int)a.scheme, j, m, a.offset, U), total) : 0.0;
            int64_t r;
            if (a.weights) {
                int64_t c = resample_search(tops.data(), 0, (int64_t)blocks, chunk_trips, (int64_t)blocks - 1, t, total);
                c = std::min<int64_t>(c, (int64_t)blocks - 1);
                r = resample_search(a.prefix, c * chunk, std::min(chunk, n - c * chunk), inner_trips, n - 1, t, total);
            } else r = resample_equal_ancestor(t, n);
            r = r < 0 ? 0 : r > n - 1 ? n - 1 : r;
            if (ancestors) { const float f = (float)r; std::memcpy(&ancestors[j], alive ? (const void*)&f : (const void*)&FM_RESAMPLE_NAN_BITS, 4); }
            for (uint32_t i = 0; i < a.n_values; ++i) {
                const uint32_t x = at<const uint32_t>(a.values[i])[r];
                at<uint32_t>(a.values_out[i])[j] = alive ? x : FM_RESAMPLE_NAN_BITS;
            }
        }
    }
    return hipSuccess;
}

} // namespace fm
