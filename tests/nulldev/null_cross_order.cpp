// null_cross_order.cpp — TEST-ONLY stand-ins for the launchers of cross_order_kernel.hip, beside the null device of tests/nulldev
// (null_hip.cpp: device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real
// work the way the kernels do it, not the way the definition states it: the K words of a path padded with (NaN key, own position) to the
// power of two the launch would use, sorted by the SAME compile-time network (fm_cross_network) on pairs or, with no index wanted, on keys
// alone; the outputs walked by sorted position through value_begin / index_begin as the kernel walks them — so that the drivers hold the
// network, the pads and the ordering of the selectors to the definition's std::sort on the CPU.  Outputs are written at their full size
// (an undersized one is an ASan report).  The select stand-in range-checks the index before it picks an address, as the kernel does.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/cross_order_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }

template <int P, bool PAIRS>
void order_paths(const DevCrossOrderArgs& a) {
    const uint32_t K = a.n_vectors;
    for (int64_t p = 0; p < a.n; ++p) {
        uint64_t pairs[P]; uint32_t keys[P];
        for (int i = 0; i < P; ++i) {
            const uint32_t key = (uint32_t)i < K ? fmhost::fm_order_key(at<const uint32_t>(a.v[i])[p]) : fmhost::FM_ORDER_NAN_KEY;
            pairs[i] = fmhost::fm_cross_pair(key, (uint32_t)i); keys[i] = key;
        }
        if (PAIRS) fmhost::fm_cross_network<P>(pairs); else fmhost::fm_cross_network<P>(keys);
        for (uint32_t r = 0; r < K; ++r) {
            const uint32_t key = PAIRS ? fmhost::fm_cross_pair_key(pairs[r]) : keys[r];
            for (uint32_t o = a.value_begin[r]; o < a.value_begin[r + 1]; ++o) at<uint32_t>(a.value_out[o])[p] = fmhost::fm_order_bits(key);
            if (PAIRS) for (uint32_t o = a.index_begin[r]; o < a.index_begin[r + 1]; ++o) at<float>(a.index_out[o])[p] = (float)fmhost::fm_cross_pair_slot(pairs[r]);
        }
    }
}
template <bool PAIRS>
void order_padded(const DevCrossOrderArgs& a) {
    switch (fmhost::fm_cross_padded((int)a.n_vectors)) {
    case 2:  order_paths<2, PAIRS>(a); break;
    case 4:  order_paths<4, PAIRS>(a); break;
    case 8:  order_paths<8, PAIRS>(a); break;
    case 16: order_paths<16, PAIRS>(a); break;
    default: order_paths<32, PAIRS>(a); break;
    }
}
}

hipError_t launch_cross_order(const DevCrossOrderArgs& a, hipStream_t) {
    if (!cross_order_shape_ok(a)) return hipErrorInvalidValue;
    if (cross_blocks(a.n, cross_paths_per_lane(fmhost::fm_cross_padded((int)a.n_vectors), a.n_indices != 0u)) < 1) return hipErrorInvalidValue;
    if (a.n_indices) order_padded<true>(a); else order_padded<false>(a);
    return hipSuccess;
}

hipError_t launch_cross_select(const DevCrossSelectArgs& a, hipStream_t) {
    if (!cross_select_shape_ok(a)) return hipErrorInvalidValue;
    for (int64_t p = 0; p < a.n; ++p) {
        const int j = fmhost::fm_cross_select_slot(at<const float>(a.index)[p], (int)a.n_vectors);
        uint32_t u = fmhost::FM_ORDER_NAN_BITS;
        if (j >= 0) u = at<const uint32_t>(a.v[j])[p];
        at<uint32_t>(a.out)[p] = u;
    }
    return hipSuccess;
}

} // namespace fm
