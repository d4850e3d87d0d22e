// mt_bm_kernel.h — host-callable launchers of the Mersenne-Twister increment kernels in mt_bm_kernel.hip: Brownian increments (DESIGN.md
// §4.9), increments with a law per stream through an inverse CDF (§4.10), and the same with the gamma and exponential laws (§4.11).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fm {

constexpr int FM_MT_STATE_WORDS = 624;
constexpr int FM_MT_BLOCK = 256;                   // threads of a workgroup
constexpr int FM_MT_TILE_FLOATS = 3200;            // floats of one of the two LDS store tiles: 16 paths of 200 step x factor vectors
constexpr int FM_MT_MIN_SEGMENT_LOG2 = 1;          // segments are an even number of words: a draw is a pair of words
constexpr int FM_MT_MAX_SEGMENT_LOG2 = 43;
constexpr int FM_MT_JUMP_LIMIT_LOG2 = 44;         // fm_mt_jump_table.hpp holds 2^0 … 2^43: every word drawn lies below 2^44

struct DevMtBmArgs {
    float*          slab;           // n_streams vectors, `stride_floats` apart (stride is a multiple of 64 floats)
    int64_t         stride_floats;
    const double*   sqrt_dt;        // [n_streams]  sqrt(dt[step of the stream]) in fp64, one entry per stream
    const uint32_t* state;          // 624 words: the seeded state jumped to the first word of local path 0
    int64_t         n_paths;        // paths held by this process
    uint32_t        n_streams;      // n_steps * n_factors: draws per path
    uint32_t        segment_log2;   // a workgroup owns the paths whose first word lies in its segment of 2^segment_log2 words
    uint32_t        tile_paths;     // paths per LDS store tile (a multiple of 4), 0: element-wise stores
    uint32_t        n_segments;     // workgroups
};

// One law of fm_mt_icdf_kernel: host/increments.hpp's IncrementLaws::Law, byte for byte (the engine uploads that array).
struct DevMtLaw {
    int32_t  kind;                  // 0 normal: inverse normal CDF(u) · a;  1 uniform: a + (b − a) · u;  2 Poisson: min { k : table[k] >= u }
                                    // fm_mt_levy_kernel only: 4 gamma: fm_inverse_gamma_cdf(a, consts, u) · b;  5 exponential: −fm_log64(1 − u) / a
    uint32_t table_len;             // Poisson: entries of the law's CDF table, the last of them 1.0; gamma: FM_GAMMA_CONSTS
    uint32_t table_offset;          // Poisson: its first entry in `tables`; gamma: the first of the shape's constants there
    uint32_t reserved;
    double   a, b;
};

struct DevMtIcdfArgs {
    DevMtBmArgs     g;              // the generation pass as above; sqrt_dt is not read
    const DevMtLaw* laws;           // [n_streams]
    const double*   tables;         // the Poisson CDF tables the laws point into, built on the host (host/increments.hpp)
    uint32_t        linear_max;     // a table of at most this many entries is searched from 0 upwards, a longer one by bisection
};

// What the generating kernels rely on in their arguments and do not check themselves; both launchers refuse anything else, and so do the
// stand-ins of the null device (tests/nulldev/null_mt.cpp), which is how the engine's arguments are pinned without a GPU.
// `icdf`: the arguments are fm_mt_icdf_kernel's (a = icdf->g).
inline bool mt_shape_ok(const DevMtBmArgs& a, const DevMtIcdfArgs* icdf = nullptr)
{
    if (!a.slab || !a.state || ((uintptr_t)a.state & 3u) || a.n_streams == 0 || a.stride_floats < a.n_paths || (a.stride_floats & 63)) return false;
    if (a.segment_log2 < (uint32_t)FM_MT_MIN_SEGMENT_LOG2 || a.segment_log2 > (uint32_t)FM_MT_MAX_SEGMENT_LOG2) return false;
    const uint64_t words = 2ull * a.n_streams * (uint64_t)a.n_paths;
    if (a.n_segments != (uint32_t)((words + (1ull << a.segment_log2) - 1) >> a.segment_log2)) return false;
    if (a.tile_paths && ((a.tile_paths & 3u) || (uint64_t)a.tile_paths * a.n_streams > (uint64_t)FM_MT_TILE_FLOATS || (uint64_t)a.tile_paths * a.n_streams < (uint64_t)FM_MT_BLOCK)) return false;
    if (!icdf) return a.sqrt_dt != nullptr;
    return !a.sqrt_dt && icdf->laws && icdf->tables && !((uintptr_t)icdf->laws & 15u) && !((uintptr_t)icdf->tables & 7u);
}

// out[0 … 624) = the state `distance` words behind in[0 … 624) (one workgroup); distance < 2^44
hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t st);
hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t st);
hipError_t launch_mt_icdf(const DevMtIcdfArgs& a, hipStream_t st);      // kinds 0, 1, 2
hipError_t launch_mt_levy(const DevMtIcdfArgs& a, hipStream_t st);      // kinds 0, 1, 2, 4, 5 (fm_mt_levy_kernel)

} // namespace fm
