// mt_generate_engine.hpp — the engine's side of the increments generated on the device from finmath-lib's MT19937 stream: Brownian increments
//  and independent increments with a law per (time step, factor) through an inverse CDF (§4.10; definition:
// host/increments.hpp).  Kernels: mt_bm_kernel.hip.  Part of runtime.cpp's translation unit (included at its end, nowhere else), like
// order_stats_engine.hpp.
//
// fmhip_bm_generate_mersenne draws n_steps·n_factors·n_paths doubles on ONE host core and uploads them; the pass here (Engine::mt_generate)
// seeds MT19937 on the host exactly as host/mersenne.hpp does (624 words), moves that state to the first word of path `path_offset` with a
// one-workgroup launch, and lets the generating kernel enter the stream at every segment: no host vector, no upload, and a shard or a rank
// generates its own block of paths without drawing what precedes it.  The vectors come from the pool as bm_generate's do (one slab, views
// into it).  Its two callers differ in what goes up in front of the state and in the kernel:
//   mt_bm_generate           sqrt(dt) per stream; fm_mt_bm_kernel.  The numbers are the host generator's (contract in mt_bm_kernel.hip).
//   mt_increments_generate   the arguments are checked and the Poisson CDF tables built and shared between equal means on the host (ONE
//                            function, fmhost::checkedIncrementLaws, which fmhip_increments_host calls too); descriptors and tables go up;
//                            fm_mt_icdf_kernel.  The device only compares a uniform with the host's table for a Poisson draw, so counts and
//                            uniform draws are the host's exactly and normal draws are under the contract of mt_bm_kernel.hip.
//                            A call with a gamma or an exponential law (§4.11) runs fm_mt_levy_kernel instead — the same pass with those
//                            two laws from host/gamma_icdf.hpp, the text the host compiles: equal draws; the constants of a shape travel
//                            with the tables.  Any other call runs the kernel it ran before.
// Which path a caller takes is the caller's choice (FMHIP_DEVICE_MERSENNE=0, FMHIP_DEVICE_INCREMENTS=0 in the mirrors), never the engine's:
// without its kernel a pass is FMHIP_ERR_UNSUPPORTED; it never draws on the host.
#include "runtime.hpp"
#include "mt_bm_kernel.h"
#include "../host/mersenne.hpp"
#include "../host/increments.hpp"

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace fm {

// WEAK, like the order-statistics launchers: a host-only build whose stand-in for the kernels does not know these still links.
hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t st) __attribute__((weak));
hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_mt_icdf(const DevMtIcdfArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_mt_levy(const DevMtIcdfArgs& a, hipStream_t st) __attribute__((weak));

static_assert(sizeof(DevMtLaw) == sizeof(fmhost::IncrementLaws::Law) && offsetof(DevMtLaw, table_offset) == offsetof(fmhost::IncrementLaws::Law, table_offset)
              && offsetof(DevMtLaw, a) == offsetof(fmhost::IncrementLaws::Law, a) && offsetof(DevMtLaw, b) == offsetof(fmhost::IncrementLaws::Law, b),
              "the engine uploads the host's descriptors as they are");

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

// The same for the increments, as an engine error
fmhost::IncrementLaws mt_increments_check(int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const int32_t* kinds, const double* a, const double* b, const fmhip_vec* out) {
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad description of the increments");
    try { return fmhost::checkedIncrementLaws(n_steps, n_factors, n_paths, path_offset, kinds, a, b); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}

void mt_increments_check_only(int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const int32_t* kinds, const double* a, const double* b, const fmhip_vec* out) {
    (void)mt_increments_check(n_steps, n_factors, n_paths, path_offset, kinds, a, b, out);
}

// fmhip_increments_host: the definition, with its complaints as engine errors
void increments_host(int32_t seed, int n_steps, int n_factors, int64_t n_paths, const int32_t* kinds, const double* a, const double* b, double* host_out) {
    try { fmhost::independentIncrements(seed, n_steps, n_factors, n_paths, kinds, a, b, host_out); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
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

// How a generation of n_streams vectors of n_paths is cut: segments (workgroups) and the paths of an LDS store tile
static DevMtBmArgs mt_shape(int64_t n_streams, int64_t n_paths) {
    const uint64_t words_per_path = 2 * (uint64_t)n_streams, words = words_per_path * (uint64_t)n_paths;
    DevMtBmArgs a{};
    a.n_paths = n_paths; a.n_streams = (uint32_t)n_streams;
    a.segment_log2 = mt_segment_log2(words, words_per_path);
    a.n_segments = (uint32_t)((words + (uint64_t(1) << a.segment_log2) - 1) >> a.segment_log2);
    a.tile_paths = (uint32_t)(FM_MT_TILE_FLOATS / n_streams);
    a.tile_paths &= a.tile_paths >= 16 ? ~15u : ~3u;                       // whole 64-byte runs where 16 paths fit, 16-byte stores where 4 do
    if (const char* e = std::getenv("FMHIP_MT_TILE")) if (e[0] == '0' && !e[1]) a.tile_paths = 0;      // measurement: element-wise stores, L2 merges the lines
    return a;
}

// The pass.  One device block  front | seeded state | moved state  goes up in one copy: `stage(host)` fills the caller's front_bytes (a
// multiple of 8), the state follows; `launch(front on the device, a)` starts the caller's kernel with `a` complete but for what it reads
// from the front.
template <class Stage, class Launch>
void Engine::mt_generate(DevMtBmArgs a, int32_t seed, int n_steps, int n_factors, int64_t path_offset, size_t front_bytes, const char* upload, Stage stage, Launch launch, fmhip_vec* out) {
    const int64_t n_paths = a.n_paths, n_streams = a.n_streams;
    const size_t state_bytes = (size_t)FM_MT_STATE_WORDS * 4;
    int64_t stride = 0;
    Buffer* slab = slab_generate(n_paths, n_streams, &stride, [&](float* vectors) {
        void* dev = nullptr; size_t dev_cap = 0;
        try {
            char* st = (char*)ensure_stage(front_bytes + state_bytes);
            stage(st);
            const fmhost::MT19937 mt((int64_t)seed);                       // the int seed of the finmath constructor, widened
            std::memcpy(st + front_bytes, mt.mt, state_bytes);
            dev = pool_.alloc(front_bytes + 2 * state_bytes, &dev_cap);
            hip_check(hipMemcpyAsync(dev, st, front_bytes + state_bytes, hipMemcpyHostToDevice, stream_), upload);
            hip_check(hipStreamSynchronize(stream_), "sync");
            const uint32_t* seeded = reinterpret_cast<const uint32_t*>((char*)dev + front_bytes);
            a.slab = vectors; a.stride_floats = stride; a.state = seeded;
            if (n_paths > 0) {
                if (path_offset > 0) {                                     // once, so that the workgroups only jump by multiples of the segment
                    uint32_t* moved = const_cast<uint32_t*>(seeded) + FM_MT_STATE_WORDS;
                    hip_check(launch_mt_jump(seeded, 2 * (uint64_t)n_streams * (uint64_t)path_offset, moved, stream_), "launch fm_mt_jump_kernel");
                    a.state = moved;
                    n_launches_++;
                }
                launch((const char*)dev, a);
                algorithmic_bytes_ += 4 * n_paths * n_streams;
                bytes_written_ += 4 * n_paths * n_streams;
                n_launches_++;
            }
        } catch (...) {
            if (dev) pool_.release(dev, dev_cap);
            throw;
        }
        pool_.release(dev, dev_cap);
    });
    slab_views(slab, stride, n_steps, n_factors, n_paths, out);
}

void Engine::mt_bm_generate(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out) {
    require_init();
    mt_bm_check(n_steps, n_factors, n_paths, path_offset, dt, out);
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    const DevMtBmArgs shape = mt_shape(n_streams, n_paths);
    if (launch_mt_bm == nullptr || launch_mt_jump == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no Mersenne-Twister kernel");
    mt_generate(shape, seed, n_steps, n_factors, path_offset, (size_t)n_streams * 8, "Mersenne-Twister state H2D",
        [&](char* st) {
            for (int i = 0; i < n_steps; ++i) {
                const double sq = std::sqrt(dt[i]);                        // as mersenneIncrements: fp64, narrowed after the product
                for (int f = 0; f < n_factors; ++f) reinterpret_cast<double*>(st)[(size_t)i * n_factors + f] = sq;
            }
        },
        [&](const char* front, DevMtBmArgs a) {
            a.sqrt_dt = reinterpret_cast<const double*>(front);
            hip_check(launch_mt_bm(a, stream_), "launch fm_mt_bm_kernel");
        }, out);
}

void Engine::mt_increments_generate(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                                    const int32_t* kinds, const double* a_in, const double* b_in, fmhip_vec* out) {
    require_init();
    const fmhost::IncrementLaws laws = mt_increments_check(n_steps, n_factors, n_paths, path_offset, kinds, a_in, b_in, out);
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    DevMtIcdfArgs a{};
    a.g = mt_shape(n_streams, n_paths);
    a.linear_max = 16;                                                     // tables of means up to about 0.5 are walked from 0, longer ones bisected
    if (const char* e = std::getenv("FMHIP_ICDF_LINEAR_MAX")) {            // measurement: 0 = always bisect, 512 = always walk
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end == e || *end || v < 0 || v > 512) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string("FMHIP_ICDF_LINEAR_MAX=") + e + ": 0 … 512");
        a.linear_max = (uint32_t)v;
    }
    bool levy = false;
    for (const fmhost::IncrementLaws::Law& L : laws.laws) levy = levy || L.kind == fmhost::LAW_GAMMA || L.kind == fmhost::LAW_EXPONENTIAL;
    if (launch_mt_icdf == nullptr || launch_mt_jump == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no inverse-CDF increment kernel");
    if (levy && launch_mt_levy == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no kernel for gamma and exponential increments");
    // in front of the state: descriptors (32 B each), tables (at least one double, so that the pointer is never a stranger's)
    const size_t law_bytes = (size_t)n_streams * sizeof(DevMtLaw), table_bytes = std::max<size_t>(laws.tables.size(), 1) * 8;
    mt_generate(a.g, seed, n_steps, n_factors, path_offset, law_bytes + table_bytes, "increment laws, tables and Mersenne-Twister state H2D",
        [&](char* st) {
            std::memcpy(st, laws.laws.data(), law_bytes);
            std::memset(st + law_bytes, 0, table_bytes);
            if (!laws.tables.empty()) std::memcpy(st + law_bytes, laws.tables.data(), laws.tables.size() * 8);
        },
        [&](const char* front, const DevMtBmArgs& g) {
            a.g = g;
            a.laws = reinterpret_cast<const DevMtLaw*>(front);
            a.tables = reinterpret_cast<const double*>(front + law_bytes);
            if (levy) hip_check(launch_mt_levy(a, stream_), "launch fm_mt_levy_kernel");
            else hip_check(launch_mt_icdf(a, stream_), "launch fm_mt_icdf_kernel");
        }, out);
}

} // namespace fm
