// nested_engine.hpp — the engine's side of the block moments and the repeat (kernels: nested_kernel.hip; definition and
// argument rules: host/block_moments.hpp).  Producing passes in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// Every other operation maps n paths to n paths or to a few numbers on the host.  Nested simulation changes the SHAPE of a sample: k inner
// paths are started from each of m outer states (repeat), and the m·k inner payoffs become m conditional means with their inner variances
// (block moments).  block_moments: the sums of m = n / block consecutive blocks of up to four vectors, in fp64 in an association that is a
// function of `block` alone; one new, materialised vector of m elements per (vector, set bit of the mask).  repeat: a new, materialised
// vector of n·each·times elements, copied bit for bit.
//
// Both: the segments' partials of large blocks in the side-pass scratch, one launch that raises the flag and is waited for.
//
// One engine, one sample: the blocks of a vector that is spread over the shards of a device list would straddle them — such a call is
// FMHIP_ERR_UNSUPPORTED (sharded.cpp).  Under an expectation communicator both calls act on this rank's own vector, as
// fmhip_vec_read_elements's positions do: the operation is local to a path's block.
#include "runtime.hpp"
#include "nested_kernel.h"

namespace fm {

static_assert(FMHIP_BLOCK_SUM == fmhost::FM_BLOCK_SUM && FMHIP_BLOCK_MEAN == fmhost::FM_BLOCK_MEAN && FMHIP_BLOCK_VARIANCE == fmhost::FM_BLOCK_VARIANCE,
              "include/fmhip.h and host/block_moments.hpp name the same outputs");

// WEAK: see pass_need_kernel (tests/nulldev/null_nested.cpp has the stand-ins).
hipError_t launch_block_moments(const DevBlockMomentsArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_repeat(const DevRepeatArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void nested_check_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, const fmhip_vec* outs) {
    if (!vs || !outs) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments: null pointer");
    if (n_vs < 1 || n_vs > fmhost::FM_BLOCK_MAX_VECTORS) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments of " + std::to_string(n_vs) + " vectors: 1 … " + std::to_string(fmhost::FM_BLOCK_MAX_VECTORS));
    pass_as_engine_error([&] { fmhost::blockCheckMask(mask); });
    if (block < 1) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments: blocks of " + std::to_string(block) + " elements (at least 1)");
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments: vs[" + std::to_string(i) + "] is no vector");
}
void nested_check_repeat(fmhip_vec v, int64_t each, int64_t times, const fmhip_vec* out) {
    if (!v) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "repeat: of a vector");
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "repeat: null pointer: out");
    if (each < 1 || times < 1) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "repeat: each = " + std::to_string(each) + ", times = " + std::to_string(times) + " (both at least 1)");
}
// fmhip_block_moments_host: the definition, with its complaints as engine errors
void block_moments_host_checked(const float* v, int64_t n, int64_t block, uint32_t mask, float* outs) {
    pass_as_engine_error([&] { fmhost::block_moments_host(v, n, block, mask, outs); });
}

void Engine::block_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, fmhip_vec* outs) {
    require_init();
    nested_check_moments(vs, n_vs, block, mask, outs);
    const int64_t n = pass_size(vs, n_vs, "block moments");
    pass_as_engine_error([&] { fmhost::blockCheckShape(n, block); });
    pass_need_kernel(launch_block_moments != nullptr && launch_sort_done != nullptr, "block-moments");
    PassHold hold;
    pass_prepare(vs, n_vs, hold, "block moments");
    const int64_t m = n / block;
    const int n_out = fmhost::fm_block_outputs(mask), total = n_vs * n_out;
    DevBlockMomentsArgs a{};
    a.n = n; a.block = block; a.n_vectors = (uint32_t)n_vs; a.mask = mask;
    PassOutputs made(this);
    for (int i = 0; i < n_vs; ++i) {
        a.v[i] = hold.ptrs[(size_t)i];
        for (int j = 0; j < n_out; ++j) a.out[i][j] = made.add(m);
    }
    // pinned: [flag]
    char* stage = (char*)ensure_stage(64);
    pass_scratch(pass_up256(8), block_partials_bytes(n, block, n_vs));
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    a.partials = reinterpret_cast<double*>(pass_other_);
    pass_launch_raising(flag, "block moments", [&] { return launch_block_moments(a, stream_); });
    algorithmic_bytes_ += 4 * n * n_vs + 4 * m * total;
    bytes_written_ += 4 * m * total;
    made.commit(outs);
}

void Engine::repeat(fmhip_vec v, int64_t each, int64_t times, fmhip_vec* out) {
    require_init();
    nested_check_repeat(v, each, times, out);
    const int64_t n = pass_size(&v, 1, "repeat");
    pass_as_engine_error([&] { fmhost::repeatCheck(n, each, times); });
    pass_need_kernel(launch_repeat != nullptr && launch_sort_done != nullptr, "repeat");
    PassHold hold;
    pass_prepare(&v, 1, hold, "repeat");
    const int64_t total = n * each * times;
    PassOutputs made(this);
    DevRepeatArgs a{};
    a.n = n; a.each = each; a.times = times; a.v = hold.ptrs[0]; a.out = made.add(total);
    char* stage = (char*)ensure_stage(64);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "repeat", [&] { return launch_repeat(a, stream_); });
    algorithmic_bytes_ += 4 * n + 4 * total;
    bytes_written_ += 4 * total;
    made.commit(out);
}

} // namespace fm
