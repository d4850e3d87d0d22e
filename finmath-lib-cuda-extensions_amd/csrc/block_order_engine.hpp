// block_order_engine.hpp — the engine's side of the block order statistics and the block sort (kernels:
// block_order_kernel.hip; definition and argument rules: host/block_order.hpp).  Producing passes in the frame of side_pass_engine.hpp
// (which says what every such pass does), beside the block moments of nested_engine.hpp: the m·k inner values of a nested simulation
// become m order statistics per selector — the quantile, the tail mean, the worst case per outer path — or come back sorted block by block.
//
// Both: one launch for every vector of the call, then the launch that raises the flag; no scratch, no staged table (ranks and ranges are
// launch arguments).  A block above FM_BLOCK_ORDER_MAX has no kernel: FMHIP_ERR_UNSUPPORTED, said before a vector is looked at.
//
// One engine, one sample: as for the block moments a device list of several shards is FMHIP_ERR_UNSUPPORTED (sharded.cpp), and under an
// expectation communicator both calls act on this rank's own vector.
#include "runtime.hpp"
#include "block_order_kernel.h"

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_block_order.cpp has the stand-in).
hipError_t launch_block_order(const DevBlockOrderArgs& a, hipStream_t st) __attribute__((weak));

static void block_order_check_length(int64_t block, const char* what) {
    if (fmhost::blockOrderTooLong(block)) throw Error(FMHIP_ERR_UNSUPPORTED, fmhost::blockOrderTooLongWhy(block, what));
}
// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT, then FMHIP_ERR_UNSUPPORTED
void block_order_check_statistics(const fmhip_vec* vs, int n_vs, int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to,
                                  int n_ranges, const fmhip_vec* outs) {
    if (!vs || !outs) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block order statistics: null pointer");
    if (n_vs < 1 || n_vs > fmhost::FM_BLOCK_ORDER_MAX_VECTORS) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block order statistics of " + std::to_string(n_vs) + " vectors: 1 … " + std::to_string(fmhost::FM_BLOCK_ORDER_MAX_VECTORS));
    pass_as_engine_error([&] { fmhost::blockOrderCheckSelectors(block, ranks, n_ranks, range_from, range_to, n_ranges); });
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block order statistics: vs[" + std::to_string(i) + "] is no vector");
    block_order_check_length(block, "block order statistics");
}
void block_order_check_sort(fmhip_vec v, int64_t block, const fmhip_vec* out) {
    if (!v) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block sort: of a vector");
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block sort: null pointer: out");
    pass_as_engine_error([&] { fmhost::blockOrderCheckBlock(block, "block sort"); });
    block_order_check_length(block, "block sort");
}
// fmhip_block_order_statistics_host, fmhip_block_sort_host: the definition, with its complaints as engine errors
void block_order_statistics_host_checked(const float* v, int64_t n, int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to,
                                         int n_ranges, float* outs) {
    if (!v || !outs) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block order statistics: null pointer");
    pass_as_engine_error([&] { fmhost::blockOrderCheckSelectors(block, ranks, n_ranks, range_from, range_to, n_ranges); fmhost::blockOrderCheckShape(n, block, "block order statistics"); });
    block_order_check_length(block, "block order statistics");
    pass_as_engine_error([&] { fmhost::block_order_statistics_host(v, n, block, ranks, n_ranks, range_from, range_to, n_ranges, outs); });
}
void block_sort_host_checked(const float* v, int64_t n, int64_t block, float* out) {
    if (!v || !out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "block sort: null pointer");
    pass_as_engine_error([&] { fmhost::blockOrderCheckShape(n, block, "block sort"); });
    block_order_check_length(block, "block sort");
    pass_as_engine_error([&] { fmhost::block_sort_host(v, n, block, out); });
}

void Engine::block_order_statistics(const fmhip_vec* vs, int n_vs, int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to,
                                    int n_ranges, fmhip_vec* outs) {
    require_init();
    block_order_check_statistics(vs, n_vs, block, ranks, n_ranks, range_from, range_to, n_ranges, outs);
    const int64_t n = pass_size(vs, n_vs, "block order statistics");
    pass_as_engine_error([&] { fmhost::blockOrderCheckShape(n, block, "block order statistics"); });
    pass_need_kernel(launch_block_order != nullptr && launch_sort_done != nullptr, "block-order");
    PassHold hold;
    pass_prepare(vs, n_vs, hold, "block order statistics");
    const int64_t m = n / block;
    const int n_out = n_ranks + n_ranges, total = n_vs * n_out;
    DevBlockOrderArgs a{};
    a.n = n; a.block = block; a.n_vectors = (uint32_t)n_vs; a.n_ranks = (uint32_t)n_ranks; a.n_ranges = (uint32_t)n_ranges; a.sort = 0u;
    for (int j = 0; j < n_ranks; ++j) a.ranks[j] = (uint32_t)ranks[j];
    for (int j = 0; j < n_ranges; ++j) { a.range_from[j] = (uint32_t)range_from[j]; a.range_to[j] = (uint32_t)range_to[j]; }
    PassOutputs made(this);
    for (int i = 0; i < n_vs; ++i) {
        a.v[i] = hold.ptrs[(size_t)i];
        for (int j = 0; j < n_out; ++j) a.out[i][j] = made.add(m);
    }
    // pinned: [flag]
    char* stage = (char*)ensure_stage(64);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "block order statistics", [&] { return launch_block_order(a, stream_); });
    algorithmic_bytes_ += 4 * n * n_vs + 4 * m * total;
    bytes_written_ += 4 * m * total;
    made.commit(outs);
}

void Engine::block_sort(fmhip_vec v, int64_t block, fmhip_vec* out) {
    require_init();
    block_order_check_sort(v, block, out);
    const int64_t n = pass_size(&v, 1, "block sort");
    pass_as_engine_error([&] { fmhost::blockOrderCheckShape(n, block, "block sort"); });
    pass_need_kernel(launch_block_order != nullptr && launch_sort_done != nullptr, "block-order");
    PassHold hold;
    pass_prepare(&v, 1, hold, "block sort");
    PassOutputs made(this);
    DevBlockOrderArgs a{};
    a.n = n; a.block = block; a.n_vectors = 1u; a.sort = 1u; a.v[0] = hold.ptrs[0]; a.out[0][0] = made.add(n);
    char* stage = (char*)ensure_stage(64);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "block sort", [&] { return launch_block_order(a, stream_); });
    algorithmic_bytes_ += 8 * n;
    bytes_written_ += 4 * n;
    made.commit(out);
}

} // namespace fm
