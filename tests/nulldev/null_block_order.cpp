// null_block_order.cpp — TEST-ONLY stand-in for the launcher of block_order_kernel.hip, beside the null device of tests/nulldev
// (null_hip.cpp: device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-in does the real
// work the way the kernels do it, not the way the definition states it: the keys of a block padded with 0xffffffff to the power of two the
// regime uses, sorted; ranks read from the padded array; a range summed as the WAVE sums it — 64 lanes walk a segment of 2048 terms from
// −0.0, the full butterfly over 64 lanes with bit 5 first, the second segment's sum added to the first's — so that the drivers hold the
// kernels' association to the definition's (fm_block_sums) on the CPU.  Outputs are written at their full size (an undersized one is an ASan
// report).  The flag is raised by launch_sort_done (null_sort.cpp).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/block_order_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }

double wave_range_sum(const uint32_t* sorted, uint32_t from, uint32_t count) {
    double S = -0.0;
    for (uint32_t s0 = 0; s0 < count; s0 += (uint32_t)fmhost::FM_BLOCK_SEGMENT) {
        const uint32_t terms = std::min<uint32_t>(count - s0, (uint32_t)fmhost::FM_BLOCK_SEGMENT);
        double lane[64];
        for (uint32_t l = 0; l < 64; ++l) {
            double x = -0.0;
            for (uint32_t k = l; k < terms; k += 64) x = x + fmhost::fm_order_term(sorted[from + s0 + k]);
            lane[l] = x;
        }
        for (uint32_t off = 32; off > 0; off >>= 1) {
            double next[64];
            for (uint32_t l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off];
            std::memcpy(lane, next, sizeof lane);
        }
        S = s0 == 0 ? lane[0] : S + lane[0];
    }
    return S;
}
}

hipError_t launch_block_order(const DevBlockOrderArgs& a, hipStream_t) {
    if (!block_order_shape_ok(a)) return hipErrorInvalidValue;
    if (order_grid(a.n, a.block) < 1) return hipErrorInvalidValue;
    const int64_t m = a.n / a.block;
    const size_t padded = order_is_small(a.block) ? (size_t)fmhost::fm_block_width(a.block) : (size_t)order_padded(a.block);
    std::vector<uint32_t> keys(padded);
    for (uint32_t slot = 0; slot < a.n_vectors; ++slot) {
        const uint32_t* v = at<const uint32_t>(a.v[slot]);
        for (int64_t q = 0; q < m; ++q) {
            for (size_t e = 0; e < padded; ++e) keys[e] = (int64_t)e < a.block ? fmhost::fm_order_key(v[q * a.block + (int64_t)e]) : fmhost::FM_ORDER_NAN_KEY;
            std::sort(keys.begin(), keys.end());
            if (a.sort) {
                for (int64_t e = 0; e < a.block; ++e) at<uint32_t>(a.out[slot][0])[q * a.block + e] = fmhost::fm_order_bits(keys[(size_t)e]);
                continue;
            }
            for (uint32_t j = 0; j < a.n_ranks; ++j) at<uint32_t>(a.out[slot][j])[q] = fmhost::fm_order_bits(keys[a.ranks[j]]);
            for (uint32_t j = 0; j < a.n_ranges; ++j) {
                const uint32_t count = a.range_to[j] - a.range_from[j] + 1u;
                at<float>(a.out[slot][a.n_ranks + j])[q] = fmhost::fm_order_mean(wave_range_sum(keys.data(), a.range_from[j], count), (int64_t)count);
            }
        }
    }
    return hipSuccess;
}

} // namespace fm
