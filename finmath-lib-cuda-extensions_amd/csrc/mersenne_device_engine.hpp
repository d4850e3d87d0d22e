// mersenne_device_engine.hpp — the engine's side of the Mersenne-Twister Brownian increments generated on the device (DESIGN.md §4.9;
// kernels: mt_bm_kernel.hip).  Part of runtime.cpp's translation unit (included at its end, nowhere else), like order_stats_engine.hpp.
//
// fmhip_bm_generate_mersenne draws n_steps·n_factors·n_paths doubles on ONE host core and uploads them; this pass seeds MT19937 on the
// host exactly as host/mersenne.hpp does (624 words), moves that state to the first word of path `path_offset` with a one-workgroup
// launch, and lets fm_mt_bm_kernel enter the stream at every segment: no host vector, no upload, and a shard or a rank generates its
// own block of paths without drawing what precedes it.  The vectors come from the pool as bm_generate's do (one slab, views into it).
// The numbers are the host generator's (contract in mt_bm_kernel.hip); which path a caller takes is the caller's choice
// (FMHIP_DEVICE_MERSENNE=0 in the mirrors), never the engine's: without the kernel this pass is FMHIP_ERR_UNSUPPORTED.
#include "runtime.hpp"
#include "mt_bm_kernel.h"
#include "../host/mersenne.hpp"

#include <cstdlib>
#include <cstring>

namespace fm {

// WEAK, like the order-statistics launchers: a host-only build whose stand-in for the kernels does not know these still links.
hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t st) __attribute__((weak));
hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t st) __attribute__((weak));

// Everything that can be said about the arguments without a device.  The stream is entered by jump-ahead over a table of 44 powers of two:
// the last word drawn lies below 2^44.
void mt_bm_check(int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, const fmhip_vec* out) {
    if (n_steps <= 0 || n_factors <= 0 || !dt || !out || path_offset < 0 || n_paths < 0 || n_paths > (int64_t(1) << 31))
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad Brownian motion description");
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    if (n_streams > (int64_t(1) << 24)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "more than 2^24 increments per path");
    for (int i = 0; i < n_steps; ++i) if (!(dt[i] >= 0.0)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "negative time step");
    const int64_t limit = (int64_t(1) << FM_MT_JUMP_LIMIT_LOG2) / (2 * n_streams);       // paths whose words all lie below 2^44
    if (path_offset > limit || n_paths > limit - path_offset)
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the Mersenne-Twister stream is entered by jump-ahead, which reaches 2^44 words: path offset + paths <= " + std::to_string(limit) + " at this shape");
}

// Segment length 2^j words: a few workgroups per CU at large sizes, one workgroup where a jump would cost more than it saves, never
// fewer than one path per workgroup.  FMHIP_MT_SEGMENT_LOG2 (tests: the numbers do not depend on it) overrides the choice.
static uint32_t mt_segment_log2(uint64_t words, uint64_t words_per_path) {
    if (const char* forced = std::getenv("FMHIP_MT_SEGMENT_LOG2")) {
        char* end = nullptr;
        const long j = std::strtol(forced, &end, 10);
        if (end == forced || *end || j < FM_MT_MIN_SEGMENT_LOG2 || j > FM_MT_MAX_SEGMENT_LOG2 || ((words + (uint64_t(1) << j) - 1) >> j) > (uint64_t(1) << 20))
            throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string("FMHIP_MT_SEGMENT_LOG2=") + forced + ": 1 … 43, and at most 2^20 segments");
        return (uint32_t)j;
    }
    uint32_t j = 15;
    while ((words >> j) > 1024) ++j;
    while ((uint64_t(1) << j) < words_per_path) ++j;
    return j;
}

void Engine::mt_bm_generate(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out) {
    require_init();
    mt_bm_check(n_steps, n_factors, n_paths, path_offset, dt, out);
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    const uint64_t words_per_path = 2 * (uint64_t)n_streams, words = words_per_path * (uint64_t)n_paths;
    DevMtBmArgs a{};
    a.n_paths = n_paths; a.n_streams = (uint32_t)n_streams;
    a.segment_log2 = mt_segment_log2(words, words_per_path);
    a.n_segments = (uint32_t)((words + (uint64_t(1) << a.segment_log2) - 1) >> a.segment_log2);
    a.tile_paths = (uint32_t)(FM_MT_TILE_FLOATS / n_streams);
    a.tile_paths &= a.tile_paths >= 16 ? ~15u : ~3u;                       // whole 64-byte runs where 16 paths fit, 16-byte stores where 4 do
    if (const char* e = std::getenv("FMHIP_MT_TILE")) if (e[0] == '0' && !e[1]) a.tile_paths = 0;      // measurement: element-wise stores, L2 merges the lines
    if (launch_mt_bm == nullptr || launch_mt_jump == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no Mersenne-Twister kernel");

    const int64_t stride = (n_paths + 63) & ~int64_t(63);                  // every vector 256-B aligned
    Buffer* slab = new_buffer(std::max<int64_t>(stride, 64) * n_streams);
    slab->refs = 0;
    void* dev = nullptr; size_t dev_cap = 0;
    const size_t sq_bytes = (size_t)n_streams * 8, state_bytes = (size_t)FM_MT_STATE_WORDS * 4;
    try {
        char* st = (char*)ensure_stage(sq_bytes + state_bytes);
        for (int i = 0; i < n_steps; ++i) {
            const double sq = std::sqrt(dt[i]);                            // as mersenneIncrements: fp64, narrowed after the product
            for (int f = 0; f < n_factors; ++f) reinterpret_cast<double*>(st)[(size_t)i * n_factors + f] = sq;
        }
        const fmhost::MT19937 mt((int64_t)seed);                           // the int seed of the finmath constructor, widened
        std::memcpy(st + sq_bytes, mt.mt, state_bytes);
        dev = pool_.alloc(sq_bytes + 2 * state_bytes, &dev_cap);
        hip_check(hipMemcpyAsync(dev, st, sq_bytes + state_bytes, hipMemcpyHostToDevice, stream_), "Mersenne-Twister state H2D");
        hip_check(hipStreamSynchronize(stream_), "sync");
        const uint32_t* seeded = reinterpret_cast<const uint32_t*>((char*)dev + sq_bytes);
        a.slab = slab->ptr; a.stride_floats = stride;
        a.sqrt_dt = (const double*)dev; a.state = seeded;
        if (n_paths > 0) {
            if (path_offset > 0) {                                         // once, so that the workgroups only jump by multiples of the segment
                uint32_t* moved = const_cast<uint32_t*>(seeded) + FM_MT_STATE_WORDS;
                hip_check(launch_mt_jump(seeded, words_per_path * (uint64_t)path_offset, moved, stream_), "launch fm_mt_jump_kernel");
                a.state = moved;
                n_launches_++;
            }
            hip_check(launch_mt_bm(a, stream_), "launch fm_mt_bm_kernel");
            algorithmic_bytes_ += 4 * n_paths * n_streams;
            bytes_written_ += 4 * n_paths * n_streams;
            n_launches_++;
        }
    } catch (...) {
        if (dev) pool_.release(dev, dev_cap);
        slab->refs = 1; buffer_unref(slab);
        throw;
    }
    pool_.release(dev, dev_cap);
    const uint32_t bm_id = next_bm_id_++;
    for (int64_t s = 0; s < n_streams; ++s) {
        Buffer* v = new Buffer();
        v->ptr = slab->ptr + s * stride; v->cap = 0; v->refs = 1; v->parent = slab;
        slab->refs++;
        Node* nd = new_node(n_paths);
        nd->buf = v;
        nd->bm_id = bm_id; nd->bm_step = (int32_t)(s / n_factors); nd->bm_steps = n_steps;
        out[s] = nd->id;
    }
}

} // namespace fm
