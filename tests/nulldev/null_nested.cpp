// null_nested.cpp — TEST-ONLY stand-ins for the two launchers of nested_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real work the plain
// way, phase by phase as the kernels do: a block of at most one segment is summed by the definition (fm_block_segment); a longer one leaves
// its segments' { s1, s2 } exactly where the block kernel writes them — [vector][block][segment] of the side-pass scratch, which is so used
// at its full size (an undersized scratch or output is an ASan report) — and the combine reads them back (fm_block_unit).  The repeat
// writes whole quads as the kernel does: the last one reaches into the padding of the output.  The flag is raised by launch_sort_done
// (null_sort.cpp).
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/nested_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
}

hipError_t launch_block_moments(const DevBlockMomentsArgs& a, hipStream_t) {
    if (!block_moments_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t m = a.n / a.block, segments = fmhost::fm_block_segments(a.block);
    for (uint32_t slot = 0; slot < a.n_vectors; ++slot) {
        const float* v = at<const float>(a.v[slot]);
        for (int64_t q = 0; q < m; ++q) {
            fmhost::BlockSums s;
            if (!block_is_large(a.block)) s = fmhost::fm_block_segment(v + q * a.block, a.block);
            else {
                double* part = a.partials + (((int64_t)slot * m + q) * segments) * 2;
                for (int64_t g = 0; g < segments; ++g) {
                    const int64_t e0 = g * fmhost::FM_BLOCK_SEGMENT, count = a.block - e0 < fmhost::FM_BLOCK_SEGMENT ? a.block - e0 : fmhost::FM_BLOCK_SEGMENT;
                    const fmhost::BlockSums p = fmhost::fm_block_segment(v + q * a.block + e0, count);
                    part[2 * g] = p.s1; part[2 * g + 1] = p.s2;
                }
                s = fmhost::fm_block_unit(part, part + 1, segments, 2);
            }
            int j = 0;
            for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1)
                if (a.mask & (uint32_t)bit) at<float>(a.out[slot][j++])[q] = fmhost::fm_block_output(bit, s, a.block);
        }
    }
    return hipSuccess;
}

hipError_t launch_repeat(const DevRepeatArgs& a, hipStream_t) {
    if (!repeat_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t* v = at<const uint32_t>(a.v);
    uint32_t* out = at<uint32_t>(a.out);
    const int64_t total = a.n * a.each * a.times, quads = (total + 3) / 4;
    for (int64_t o = 0; o < quads * 4; ++o) out[o] = v[(o / a.each) % a.n];
    return hipSuccess;
}

} // namespace fm
