// resample_kernel.h — host-callable launcher of the kernels of resample_kernel.hip (engine side: resample_engine.hpp):
// m ancestors drawn from n weights, up to 8 companion vectors gathered along.  The definition, and every function of it that the kernels
// call, is resample_host.hpp's (no HIP in it: tests/cpp/test_resample_host.cpp drives it on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "resample_host.hpp"

namespace fm {

constexpr int FM_RESAMPLE_BLOCK = 256;              // lanes of a gather workgroup
constexpr int FM_RESAMPLE_ITEMS = 4;                // outputs per lane, FM_RESAMPLE_BLOCK apart: every store of a wave is 256 contiguous bytes
constexpr int FM_RESAMPLE_TILE = FM_RESAMPLE_BLOCK * FM_RESAMPLE_ITEMS;

// Device scratch of a weighted call (the side-pass scratch that need not be zero), 256-byte aligned parts:
//   totals  [blocks]      the total of chunk c inside the chunk       written by the totals kernel
//   bases   [blocks + 1]  the base of chunk c (entry 0 is not used), then the total P[n-1]: bases[c + 1] is the LAST prefix of chunk c
constexpr size_t resample_totals_bytes(int64_t n) { return prefix_up256((size_t)prefix_blocks(n) * 8); }
constexpr size_t resample_scratch_bytes(int64_t n) { return resample_totals_bytes(n) + prefix_up256(((size_t)prefix_blocks(n) + 1) * 8); }
constexpr int64_t resample_prefix_floats(int64_t n) { return 2 * n; }       // the temporary of P: 8n bytes, in floats of the pool

struct DevResampleArgs {
    uint32_t  n, m;
    uint32_t  chunk_tiles;     // prefix_chunk_tiles(n)
    uint32_t  scheme;          // FM_RESAMPLE_*
    uint32_t  n_values;        // 0 … FM_RESAMPLE_MAX_VALUES
    uint32_t  pad;
    double    offset;          // SYSTEMATIC
    uint64_t  weights;         // n floats, or 0: equal weights — no prefix launch, no scratch, no temporary
    uint64_t  uniforms;        // m floats (0 with SYSTEMATIC)
    uint64_t  values[FM_RESAMPLE_MAX_VALUES], values_out[FM_RESAMPLE_MAX_VALUES];       // n resp. m floats
    uint64_t  ancestors_out;   // m floats, or 0
    double*   prefix;          // device: P, n doubles (weighted)
    char*     scratch;         // device: resample_scratch_bytes(n) (weighted)
    double*   total_host;      // pinned; may be null: P[n-1] (weighted; with equal weights the engine knows it)
};
inline bool resample_shape_ok(const DevResampleArgs& a)
{
    if (!(a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.m > 0 && a.m <= (uint32_t)FM_PREFIX_MAX_N && a.scheme <= 2u && a.n_values <= (uint32_t)FM_RESAMPLE_MAX_VALUES)) return false;
    if (a.n_values == 0u && !a.ancestors_out) return false;
    if (a.ancestors_out && a.n > (uint32_t)FM_RESAMPLE_MAX_ANCESTOR_N) return false;
    if (a.scheme != (uint32_t)FM_RESAMPLE_SYSTEMATIC && !a.uniforms) return false;
    if (a.scheme == (uint32_t)FM_RESAMPLE_SYSTEMATIC && !(a.offset >= 0.0 && a.offset < 1.0)) return false;
    for (uint32_t i = 0; i < a.n_values; ++i) if (!a.values[i] || !a.values_out[i]) return false;
    return a.weights ? a.chunk_tiles == prefix_chunk_tiles(a.n) && a.prefix && a.scratch : true;
}
#if defined(__HIP__)
#define FM_RESAMPLE_ARGS_HD __host__ __device__
#else
#define FM_RESAMPLE_ARGS_HD
#endif
FM_RESAMPLE_ARGS_HD inline double* resample_totals(const DevResampleArgs& a) { return reinterpret_cast<double*>(a.scratch); }
FM_RESAMPLE_ARGS_HD inline double* resample_bases(const DevResampleArgs& a) { return reinterpret_cast<double*>(a.scratch + resample_totals_bytes(a.n)); }

// weighted: totals → carry → prefixes (P into a.prefix) → gather; equal weights: the gather alone.  Chained on `st`.
hipError_t launch_resample(const DevResampleArgs& a, hipStream_t st);

} // namespace fm
