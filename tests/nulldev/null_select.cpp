// null_select.cpp — TEST-ONLY stand-ins for the launchers of select_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real work phase by
// phase as the kernels do: every chunk of the mask is counted on its own and leaves its count where the count kernel writes it; the carry
// is the serial chain over the counts, written where the carry kernel writes it, the count into the pinned word; the compress and the
// expand read the bases back from the scratch and walk their chunks tile by tile and lane by lane — eight bits per lane, the running base,
// the bound check before every store (dst < count) and the clamp before every load; the gather walks its tiles of FM_SELECT_TILE outputs.
// So the scratch and the padded quads that the 16-byte loads reach are touched (an undersized buffer is an ASan report).  The flag is
// raised by launch_sort_done (null_sort.cpp).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/select_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
uint32_t last_of_quads(uint32_t n) { return ((n + 3u) & ~3u) - 1u; }      // storage is padded to 256 bytes: the kernels read whole quads
void touch(uint64_t address, uint32_t n) { (void)*(volatile const float*)&at<const float>(address)[last_of_quads(n)]; }
uint32_t lane_bits(const float* mask, int64_t e0, int64_t n)
{
    uint32_t bits = 0u;
    for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (e0 + i < n && select_selected(mask[e0 + i])) bits |= 1u << i;
    return bits;
}
// f(e0, bits, q0) for every lane of every tile of every chunk, q0: the selected elements before the lane's
template <class F> void walk(const DevCompressArgs& a, F f)
{
    const int64_t n = (int64_t)a.n;
    const float* mask = at<const float>(a.mask);
    const uint32_t* bases = select_bases(a);
    for (uint32_t c = 0; c < prefix_blocks(n); ++c) {
        uint32_t run = bases[c];
        for (int64_t tile = (int64_t)c * a.chunk_tiles; tile < (int64_t)(c + 1) * a.chunk_tiles && tile < prefix_tiles(n); ++tile)
            for (int lane = 0; lane < FM_PREFIX_BLOCK; ++lane) {
                const int64_t e0 = tile * FM_PREFIX_TILE + (int64_t)lane * FM_PREFIX_ITEMS;
                const uint32_t bits = lane_bits(mask, e0, n);
                f(e0, bits, run);
                run += (uint32_t)__builtin_popcount(bits);
            }
    }
}
}

hipError_t launch_select_count(const DevCompressArgs& a, hipStream_t) {
    if (!select_count_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)a.n, chunk = prefix_chunk_elems(n);
    const uint32_t blocks = prefix_blocks(n);
    const float* mask = at<const float>(a.mask);
    touch(a.mask, a.n);
    uint32_t* counts = select_counts(a);
    uint32_t* bases = select_bases(a);
    for (uint32_t c = 0; c < blocks; ++c) {
        uint32_t k = 0u;
        for (int64_t r = (int64_t)c * chunk; r < std::min<int64_t>((int64_t)(c + 1) * chunk, n); ++r) k += select_selected(mask[r]) ? 1u : 0u;
        counts[c] = k;
    }
    uint32_t run = 0u;
    for (uint32_t c = 0; c < blocks; ++c) { bases[c] = run; run += counts[c]; }
    bases[blocks] = run;
    *a.count_host = (uint64_t)run;
    return hipSuccess;
}

hipError_t launch_select_compress(const DevCompressArgs& a, hipStream_t) {
    if (!select_shape_ok(a, false)) return hipErrorInvalidValue;
    touch(a.mask, a.n);
    for (uint32_t v = 0; v < a.n_values; ++v) touch(a.values[v], a.n);
    walk(a, [&](int64_t e0, uint32_t bits, uint32_t q0) {
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
            const uint32_t dst = q0 + (uint32_t)__builtin_popcount(bits & ((1u << i) - 1u));
            if (!(bits >> i & 1u) || dst >= a.count) continue;
            if (a.positions_out) { const float f = (float)(e0 + i); std::memcpy(&at<uint32_t>(a.positions_out)[dst], &f, 4); }
            for (uint32_t v = 0; v < a.n_values; ++v) at<uint32_t>(a.values_out[v])[dst] = at<const uint32_t>(a.values[v])[e0 + i];
        }
    });
    return hipSuccess;
}

hipError_t launch_select_expand(const DevCompressArgs& a, hipStream_t) {
    if (!select_shape_ok(a, true)) return hipErrorInvalidValue;
    touch(a.mask, a.n);
    uint32_t fill; std::memcpy(&fill, &a.fill, 4);
    const uint32_t last = a.count - 1u;
    walk(a, [&](int64_t e0, uint32_t bits, uint32_t q0) {
        for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
            if (e0 + i >= (int64_t)a.n) break;
            const uint32_t q = q0 + (uint32_t)__builtin_popcount(bits & ((1u << i) - 1u));
            for (uint32_t v = 0; v < a.n_values; ++v) {
                const uint32_t x = at<const uint32_t>(a.values[v])[q < last ? q : last];
                at<uint32_t>(a.values_out[v])[e0 + i] = (bits >> i & 1u) ? x : fill;
            }
        }
    });
    return hipSuccess;
}

hipError_t launch_select_gather(const DevIndexGatherArgs& a, hipStream_t) {
    if (!gather_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)a.n, m = (int64_t)a.m;
    const float* index = at<const float>(a.index);
    for (int64_t tile = 0; tile * FM_SELECT_TILE < m; ++tile)
        for (int64_t j = tile * FM_SELECT_TILE; j < std::min<int64_t>((tile + 1) * FM_SELECT_TILE, m); ++j) {
            int64_t k = select_index(index[j], n);
            const bool alive = k >= 0;
            k = k < 0 ? 0 : k > n - 1 ? n - 1 : k;
            for (uint32_t v = 0; v < a.n_values; ++v) {
                const uint32_t x = at<const uint32_t>(a.values[v])[k];
                at<uint32_t>(a.values_out[v])[j] = alive ? x : FM_SELECT_NAN_BITS;
            }
        }
    return hipSuccess;
}

} // namespace fm
