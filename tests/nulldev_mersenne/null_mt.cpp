// null_mt.cpp — TEST-ONLY stand-in for the launchers of mt_bm_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp: device
// memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-in does what the kernels do the plain
// way: the jump with host/mt_jump.hpp, the increments one after the other with host/mersenne.hpp from the state it is handed — so the
// driver can check against fmhip_mersenne_increments that the engine seeds, jumps (path offsets, shards) and lays the vectors out as the
// kernel expects, and a wild or undersized pointer is an ASan report.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/mt_bm_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/mt_jump.hpp"

namespace fm {

hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t) {
    if (!in || !out || in == out) return hipErrorInvalidValue;
    std::memcpy(out, in, sizeof(uint32_t) * FM_MT_STATE_WORDS);
    try { fmhost::mtJump(out, distance); } catch (...) { return hipErrorInvalidValue; }
    return hipSuccess;
}

hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t) {
    if (a.n_paths <= 0) return hipSuccess;
    if (!a.slab || !a.sqrt_dt || !a.state || a.n_streams == 0 || a.stride_floats < a.n_paths || (a.stride_floats & 63)) return hipErrorInvalidValue;
    if (a.segment_log2 < (uint32_t)FM_MT_MIN_SEGMENT_LOG2 || a.segment_log2 > (uint32_t)FM_MT_MAX_SEGMENT_LOG2) return hipErrorInvalidValue;
    const uint64_t words = 2ull * a.n_streams * (uint64_t)a.n_paths;
    if (a.n_segments != (uint32_t)((words + (1ull << a.segment_log2) - 1) >> a.segment_log2)) return hipErrorInvalidValue;
    if (a.tile_paths && ((a.tile_paths & 3u) || (uint64_t)a.tile_paths * a.n_streams > (uint64_t)FM_MT_TILE_FLOATS || (uint64_t)a.tile_paths * a.n_streams < 256u)) return hipErrorInvalidValue;
    fmhost::MT19937 mt((int64_t)0);
    std::memcpy(mt.mt, a.state, sizeof mt.mt);
    mt.mti = 624;
    for (int64_t p = 0; p < a.n_paths; ++p)
        for (uint32_t s = 0; s < a.n_streams; ++s)
            a.slab[(size_t)s * a.stride_floats + p] = (float)(fmhost::inverseNormalCdf(mt.nextDouble()) * a.sqrt_dt[s]);
    return hipSuccess;
}

} // namespace fm
