// null_sort.cpp — TEST-ONLY stand-ins for the five launchers of sort_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real work the
// plain way: a pass is a stable counting pass on the digit of the key (os::key_of for the float vector of the first pass), workgroup by
// workgroup over the chunks of sort_chunk_tiles / sort_blocks, with the count table written exactly where the kernels write it — counts,
// then first destinations in (digit, workgroup) order (sort_offsets_host) — so the engine's table and ping-pong buffers are used at their
// full size: table[blocks·256 − 1] and the last element of every source and destination are touched, the padded quad the 16-byte loads
// and stores reach among them (an undersized table or buffer is an ASan report).  Gather, scores and read-elements run as the kernels
// define them; launch_sort_done raises the flag.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/sort_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
uint32_t last_of_quads(uint32_t n) { return ((n + 3u) & ~3u) - 1u; }      // storage is padded to 256 bytes: the kernels read and write whole quads
}

hipError_t launch_sort_pass(const DevSortPassArgs& a, hipStream_t) {
    if (!sort_pass_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t n = a.n, blocks = sort_blocks((int64_t)n);
    const uint64_t chunk = (uint64_t)a.chunk_tiles * FM_SORT_TILE;
    const uint32_t* src_key = at<const uint32_t>(a.src_key);
    const uint32_t* src_idx = a.from_floats ? nullptr : at<const uint32_t>(a.src_idx);
    uint32_t* dst_key = a.write_keys ? at<uint32_t>(a.dst_key) : nullptr;
    uint32_t* dst_idx = at<uint32_t>(a.dst_idx);
    (void)*(volatile const uint32_t*)&src_key[last_of_quads(n)];
    if (src_idx) (void)*(volatile const uint32_t*)&src_idx[n - 1u];
    if (dst_key) dst_key[n - 1u] = 0u;
    dst_idx[n - 1u] = 0u;
    a.table[(size_t)blocks * FM_SORT_BINS - 1] = 0u;
    auto key_of = [&](uint64_t e) { uint32_t k = src_key[e]; if (a.from_floats) { float x; std::memcpy(&x, &k, 4); k = os::key_of(x); } return k; };
    // count: workgroup w, its chunk of the current order
    for (uint32_t w = 0; w < blocks; ++w) {
        uint32_t* row = a.table + (size_t)w * FM_SORT_BINS;
        for (int d = 0; d < FM_SORT_BINS; ++d) row[d] = 0u;
        const uint64_t e1 = (w + 1u) * chunk < n ? (w + 1u) * chunk : n;
        for (uint64_t e = w * chunk; e < e1; ++e) row[(key_of(e) >> a.shift) & 255u]++;
    }
    sort_offsets_host(a.table, blocks);
    // scatter: workgroup w walks its chunk in order from its row of first destinations (kept in registers: the table is not written again)
    for (uint32_t w = 0; w < blocks; ++w) {
        uint32_t run[FM_SORT_BINS];
        std::memcpy(run, a.table + (size_t)w * FM_SORT_BINS, sizeof run);
        const uint64_t e1 = (w + 1u) * chunk < n ? (w + 1u) * chunk : n;
        for (uint64_t e = w * chunk; e < e1; ++e) {
            const uint32_t k = key_of(e), to = run[(k >> a.shift) & 255u]++;
            if (to >= n) return hipErrorInvalidValue;
            if (dst_key) dst_key[to] = k;
            dst_idx[to] = src_idx ? src_idx[e] : (uint32_t)e;
        }
    }
    return hipSuccess;
}

hipError_t launch_sort_gather(const DevSortGatherArgs& a, hipStream_t) {
    if (a.n == 0u || a.n > (uint32_t)FM_SORT_MAX_N || a.count == 0u || a.count > 1u + (uint32_t)FM_SORT_MAX_VALUES || !a.perm) return hipErrorInvalidValue;
    const uint32_t* perm = at<const uint32_t>(a.perm);
    (void)*(volatile const uint32_t*)&perm[last_of_quads(a.n)];
    for (uint32_t k = 0; k < a.count; ++k) {
        if (!a.src[k] || !a.dst[k] || a.src[k] == a.dst[k]) return hipErrorInvalidValue;
        const uint32_t* src = at<const uint32_t>(a.src[k]);
        uint32_t* dst = at<uint32_t>(a.dst[k]);
        dst[last_of_quads(a.n)] = 0u;
        for (uint32_t r = 0; r < a.n; ++r) { if (perm[r] >= a.n) return hipErrorInvalidValue; dst[r] = src[perm[r]]; }
    }
    return hipSuccess;
}

hipError_t launch_sort_scores(uint64_t perm_at, uint64_t out_at, uint32_t n, hipStream_t) {
    if (n == 0u || n > (uint32_t)FM_SORT_MAX_N || !perm_at || !out_at) return hipErrorInvalidValue;
    const uint32_t* perm = at<const uint32_t>(perm_at);
    float* out = at<float>(out_at);
    (void)*(volatile const uint32_t*)&perm[last_of_quads(n)];
    for (uint32_t r = 0; r < n; ++r) { if (perm[r] >= n) return hipErrorInvalidValue; out[perm[r]] = (float)(((double)r + 0.5) / (double)n); }
    return hipSuccess;
}

hipError_t launch_sort_read_elements(uint64_t v, const uint32_t* pos, uint32_t count, double* out_host, hipStream_t) {
    if (!v || !pos || count == 0u || !out_host) return hipErrorInvalidValue;
    const float* x = at<const float>(v);
    for (uint32_t j = 0; j < count; ++j) out_host[j] = (double)x[pos[j]];
    return hipSuccess;
}

hipError_t launch_sort_done(uint64_t* done_flag, uint64_t done_value, hipStream_t) {
    if (!done_flag) return hipErrorInvalidValue;
    __atomic_store_n(done_flag, done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

} // namespace fm
