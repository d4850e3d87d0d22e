// nested_engine.hpp — the engine's side of the block moments and the repeat (kernels: nested_kernel.hip; definition and
// argument rules: host/block_moments.hpp).  Part of runtime.cpp's translation unit (included at its end behind side_pass_engine.hpp,
// nowhere else).
//
// Every other operation maps n paths to n paths or to a few numbers on the host.  Nested simulation changes the SHAPE of a sample: k inner
// paths are started from each of m outer states (repeat), and the m·k inner payoffs become m conditional means with their inner variances
// (block moments).  block_moments: the sums of m = n / block consecutive blocks of up to four vectors, in fp64 in an association that is a
// function of `block` alone; one new, materialised vector of m elements per (vector, set bit of the mask).  repeat: a new, materialised
// vector of n·each·times elements, copied bit for bit.
//
// Both stand in the frame of side_pass_engine.hpp: arguments checked before anything is flushed or launched, one flush, the vectors'
// storage held, the segments' partials of large blocks in the side-pass scratch, the outputs allocated before the launch (a failed
// allocation leaves nothing launched and gives the earlier buffers back), ONE pass_launch whose chain ends in the kernel that raises the
// flag, the wait under the engine lock.
//
// One engine, one sample: the blocks of a vector that is spread over the shards of a device list would straddle them — such a call is
// FMHIP_ERR_UNSUPPORTED (sharded.cpp).  Under an expectation communicator both calls act on this rank's own vector, as
// fmhip_vec_read_elements's positions do: the operation is local to a path's block.  Without the kernels a call is FMHIP_ERR_UNSUPPORTED:
// the mirrors' host path is a caller's choice (FMHIP_DEVICE_NESTED=0), never the engine's.
#include "runtime.hpp"
#include "nested_kernel.h"

namespace fm {

static_assert(FMHIP_BLOCK_SUM == fmhost::FM_BLOCK_SUM && FMHIP_BLOCK_MEAN == fmhost::FM_BLOCK_MEAN && FMHIP_BLOCK_VARIANCE == fmhost::FM_BLOCK_VARIANCE,
              "include/fmhip.h and host/block_moments.hpp name the same outputs");

// WEAK: see pass_need_kernel (tests/nulldev/null_nested.cpp has the stand-ins; launch_sort_done, the one-lane kernel that raises the flag,
// is declared weak in sort_engine.hpp).
hipError_t launch_block_moments(const DevBlockMomentsArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_repeat(const DevRepeatArgs& a, hipStream_t st) __attribute__((weak));

template <class F> static void nested_as_engine_error(F&& f) {
    try { f(); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}
// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void nested_check_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, const fmhip_vec* outs) {
    if (!vs || !outs) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments: null pointer");
    if (n_vs < 1 || n_vs > fmhost::FM_BLOCK_MAX_VECTORS) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block moments of " + std::to_string(n_vs) + " vectors: 1 … " + std::to_string(fmhost::FM_BLOCK_MAX_VECTORS));
    nested_as_engine_error([&] { fmhost::blockCheckMask(mask); });
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
    nested_as_engine_error([&] { fmhost::block_moments_host(v, n, block, mask, outs); });
}

void Engine::block_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, fmhip_vec* outs) {
    require_init();
    nested_check_moments(vs, n_vs, block, mask, outs);
    const int64_t n = pass_size(vs, n_vs, "block moments");
    nested_as_engine_error([&] { fmhost::blockCheckShape(n, block); });
    pass_need_kernel(launch_block_moments != nullptr && launch_sort_done != nullptr, "block-moments");
    PassHold hold;
    pass_prepare(vs, n_vs, hold, "block moments");
    const int64_t m = n / block;
    const int n_out = fmhost::fm_block_outputs(mask), total = n_vs * n_out;
    DevBlockMomentsArgs a{};
    a.n = n; a.block = block; a.n_vectors = (uint32_t)n_vs; a.mask = mask;
    // the outputs first: an allocation that fails leaves nothing launched
    struct Outs { Engine* e; Buffer* b[fmhost::FM_BLOCK_MAX_VECTORS * fmhost::FM_BLOCK_MAX_OUTPUTS] = {}; ~Outs() { for (Buffer* p : b) if (p) e->buffer_unref(p); } } keep{ this };
    for (int i = 0; i < n_vs; ++i) {
        a.v[i] = hold.ptrs[(size_t)i];
        for (int j = 0; j < n_out; ++j) { keep.b[i * n_out + j] = new_buffer(m); a.out[i][j] = (uint64_t)(uintptr_t)keep.b[i * n_out + j]->ptr; }
    }
    // pinned: [flag]
    char* stage = (char*)ensure_stage(64);
    pass_scratch(pass_up256(8), block_partials_bytes(n, block, n_vs));
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    a.partials = reinterpret_cast<double*>(pass_other_);
    uint64_t* done_flag = nullptr; uint64_t done_value = 0;
    pass_launch(flag, done_flag, done_value, "block moments", [&] {
        hipError_t e = launch_block_moments(a, stream_);
        if (e == hipSuccess) e = launch_sort_done(done_flag, done_value, stream_);
        return e;
    });
    algorithmic_bytes_ += 4 * n * n_vs + 4 * m * total;
    bytes_written_ += 4 * m * total;
    for (int k = 0; k < total; ++k) {
        Node* nd = new_node(m);
        nd->buf = keep.b[k];
        keep.b[k] = nullptr;
        outs[k] = nd->id;
    }
}

fmhip_vec Engine::repeat(fmhip_vec v, int64_t each, int64_t times, const fmhip_vec* out_checked) {
    require_init();
    nested_check_repeat(v, each, times, out_checked);
    const int64_t n = pass_size(&v, 1, "repeat");
    nested_as_engine_error([&] { fmhost::repeatCheck(n, each, times); });
    pass_need_kernel(launch_repeat != nullptr && launch_sort_done != nullptr, "repeat");
    PassHold hold;
    pass_prepare(&v, 1, hold, "repeat");
    const int64_t total = n * each * times;
    Buffer* out = new_buffer(total);
    struct Out { Engine* e; Buffer*& b; ~Out() { if (b) e->buffer_unref(b); } } keep{ this, out };
    char* stage = (char*)ensure_stage(64);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    DevRepeatArgs a{};
    a.n = n; a.each = each; a.times = times; a.v = hold.ptrs[0]; a.out = (uint64_t)(uintptr_t)out->ptr;
    uint64_t* done_flag = nullptr; uint64_t done_value = 0;
    pass_launch(flag, done_flag, done_value, "repeat", [&] {
        hipError_t e = launch_repeat(a, stream_);
        if (e == hipSuccess) e = launch_sort_done(done_flag, done_value, stream_);
        return e;
    });
    algorithmic_bytes_ += 4 * n + 4 * total;
    bytes_written_ += 4 * total;
    Node* nd = new_node(total);
    nd->buf = out;
    out = nullptr;
    return nd->id;
}

} // namespace fm
