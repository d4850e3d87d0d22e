// increments_device_engine.hpp — the engine's side of independent increments with a law per (time step, factor), generated on the device
// from finmath-lib's MT19937 stream (kernel: fm_mt_icdf_kernel in mt_bm_kernel.hip; definition: host/increments.hpp).
// Part of runtime.cpp's translation unit (included at its end, behind mersenne_device_engine.hpp, whose segment choice it shares).
//
// The pass is mt_bm_generate's with a law per stream in place of sqrt(dt): the arguments are checked and the Poisson CDF tables built
// and shared between equal means on the host (ONE function, fmhost::checkedIncrementLaws, which fmhip_increments_host calls too), the
// descriptors, the tables and the seeded state go up in one copy, the state is moved to the first word of path `path_offset` by a
// one-workgroup launch, and every workgroup of fm_mt_icdf_kernel enters the stream at its segment.  The device only compares a uniform
// with the host's table for a Poisson draw, so counts and uniform draws are the host's exactly and normal draws are under the contract of
// mt_bm_kernel.hip.  Without the kernel this pass is FMHIP_ERR_UNSUPPORTED; it never draws on the host.
#include "runtime.hpp"
#include "mt_bm_kernel.h"
#include "../host/increments.hpp"

#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace fm {

hipError_t launch_mt_icdf(const DevMtIcdfArgs& a, hipStream_t st) __attribute__((weak));

static_assert(sizeof(DevMtLaw) == sizeof(fmhost::IncrementLaws::Law) && offsetof(DevMtLaw, table_offset) == offsetof(fmhost::IncrementLaws::Law, table_offset)
              && offsetof(DevMtLaw, a) == offsetof(fmhost::IncrementLaws::Law, a) && offsetof(DevMtLaw, b) == offsetof(fmhost::IncrementLaws::Law, b),
              "the engine uploads the host's descriptors as they are");

// Everything that can be said about the arguments without a device, as an engine error
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

void Engine::mt_increments_generate(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                                    const int32_t* kinds, const double* a_in, const double* b_in, fmhip_vec* out) {
    require_init();
    const fmhost::IncrementLaws laws = mt_increments_check(n_steps, n_factors, n_paths, path_offset, kinds, a_in, b_in, out);
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    const uint64_t words_per_path = 2 * (uint64_t)n_streams, words = words_per_path * (uint64_t)n_paths;
    DevMtIcdfArgs a{};
    a.g.n_paths = n_paths; a.g.n_streams = (uint32_t)n_streams;
    a.g.segment_log2 = mt_segment_log2(words, words_per_path);
    a.g.n_segments = (uint32_t)((words + (uint64_t(1) << a.g.segment_log2) - 1) >> a.g.segment_log2);
    a.g.tile_paths = (uint32_t)(FM_MT_TILE_FLOATS / n_streams);
    a.g.tile_paths &= a.g.tile_paths >= 16 ? ~15u : ~3u;                   // as mt_bm_generate
    if (const char* e = std::getenv("FMHIP_MT_TILE")) if (e[0] == '0' && !e[1]) a.g.tile_paths = 0;
    a.linear_max = 16;                                                     // tables of means up to about 0.5 are walked from 0, longer ones bisected
    if (const char* e = std::getenv("FMHIP_ICDF_LINEAR_MAX")) {            // measurement: 0 = always bisect, 512 = always walk
        char* end = nullptr;
        const long v = std::strtol(e, &end, 10);
        if (end == e || *end || v < 0 || v > 512) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string("FMHIP_ICDF_LINEAR_MAX=") + e + ": 0 … 512");
        a.linear_max = (uint32_t)v;
    }
    if (launch_mt_icdf == nullptr || launch_mt_jump == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no inverse-CDF increment kernel");

    const int64_t stride = (n_paths + 63) & ~int64_t(63);                  // every vector 256-B aligned
    Buffer* slab = new_buffer(std::max<int64_t>(stride, 64) * n_streams);
    slab->refs = 0;
    void* dev = nullptr; size_t dev_cap = 0;
    // one block: descriptors (32 B each), tables (at least one double, so that the pointer is never a stranger's), seeded state, moved state
    const size_t law_bytes = (size_t)n_streams * sizeof(DevMtLaw), table_bytes = std::max<size_t>(laws.tables.size(), 1) * 8, state_bytes = (size_t)FM_MT_STATE_WORDS * 4;
    try {
        char* st = (char*)ensure_stage(law_bytes + table_bytes + state_bytes);
        std::memcpy(st, laws.laws.data(), law_bytes);
        std::memset(st + law_bytes, 0, table_bytes);
        if (!laws.tables.empty()) std::memcpy(st + law_bytes, laws.tables.data(), laws.tables.size() * 8);
        const fmhost::MT19937 mt((int64_t)seed);                           // the int seed of the finmath constructor, widened
        std::memcpy(st + law_bytes + table_bytes, mt.mt, state_bytes);
        dev = pool_.alloc(law_bytes + table_bytes + 2 * state_bytes, &dev_cap);
        hip_check(hipMemcpyAsync(dev, st, law_bytes + table_bytes + state_bytes, hipMemcpyHostToDevice, stream_), "increment laws, tables and Mersenne-Twister state H2D");
        hip_check(hipStreamSynchronize(stream_), "sync");
        const uint32_t* seeded = reinterpret_cast<const uint32_t*>((char*)dev + law_bytes + table_bytes);
        a.g.slab = slab->ptr; a.g.stride_floats = stride;
        a.g.sqrt_dt = nullptr; a.g.state = seeded;
        a.laws = reinterpret_cast<const DevMtLaw*>(dev);
        a.tables = reinterpret_cast<const double*>((char*)dev + law_bytes);
        if (n_paths > 0) {
            if (path_offset > 0) {                                         // once, so that the workgroups only jump by multiples of the segment
                uint32_t* moved = const_cast<uint32_t*>(seeded) + FM_MT_STATE_WORDS;
                hip_check(launch_mt_jump(seeded, words_per_path * (uint64_t)path_offset, moved, stream_), "launch fm_mt_jump_kernel");
                a.g.state = moved;
                n_launches_++;
            }
            hip_check(launch_mt_icdf(a, stream_), "launch fm_mt_icdf_kernel");
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
