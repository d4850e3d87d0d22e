// cross_order_engine.hpp — the engine's side of the order statistics across vectors and of the selection behind their index (DESIGN.md
// §4.24; kernels: cross_order_kernel.hip; definition and argument rules: host/cross_order.hpp).  Producing passes in the frame of
// side_pass_engine.hpp (which says what every such pass does), beside the named functions of analytic_engine.hpp: the K values of every
// path — the assets of a basket — are sorted per path, and the ranks a call selects come back as new vectors, as values, as slots or both.
//
// Both: one launch, not waited for; nothing goes through the pinned stage — the selectors, ordered by rank, are the launch's arguments.
// The passes are elementwise: a device list runs them per shard (sharded.cpp), a communicator's ranks each on their own paths.
#include "runtime.hpp"
#include "cross_order_kernel.h"

namespace fm {

static_assert(FMHIP_CROSS_VALUES == fmhost::FM_CROSS_VALUES && FMHIP_CROSS_INDICES == fmhost::FM_CROSS_INDICES,
              "include/fmhip.h and host/cross_order.hpp name the same outputs");

// WEAK: see pass_need_kernel (tests/nulldev/null_cross_order.cpp has the stand-ins).
hipError_t launch_cross_order(const DevCrossOrderArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_cross_select(const DevCrossSelectArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void cross_order_check_statistics(const fmhip_vec* vs, int n_vs, const int* ranks, int n_ranks, int outputs, const fmhip_vec* outs) {
    if (!vs || !outs) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross order statistics: null pointer");
    pass_as_engine_error([&] { fmhost::crossOrderCheck(n_vs, ranks, n_ranks, outputs); });
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross order statistics: vs[" + std::to_string(i) + "] is no vector");
}
void cross_order_check_select(fmhip_vec index, const fmhip_vec* vs, int n_vs, const fmhip_vec* out) {
    if (!index) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross select: by an index vector");
    if (!vs || !out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross select: null pointer");
    pass_as_engine_error([&] { fmhost::crossSelectCheck(n_vs); });
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross select: vs[" + std::to_string(i) + "] is no vector");
}
// fmhip_cross_order_statistics_host, fmhip_cross_select_host: the definition, with its complaints as engine errors
void cross_order_statistics_host_checked(const float* const* vs, int n_vs, int64_t n, const int* ranks, int n_ranks, int outputs, float* const* outs) {
    pass_as_engine_error([&] { fmhost::cross_order_statistics_host(vs, n_vs, n, ranks, n_ranks, outputs, outs); });
}
void cross_select_host_checked(const float* index, const float* const* vs, int n_vs, int64_t n, float* out) {
    pass_as_engine_error([&] { fmhost::cross_select_host(index, vs, n_vs, n, out); });
}

void Engine::cross_order_statistics(const fmhip_vec* vs, int n_vs, const int* ranks, int n_ranks, int outputs, fmhip_vec* outs) {
    require_init();
    cross_order_check_statistics(vs, n_vs, ranks, n_ranks, outputs, outs);
    pass_size(vs, n_vs, "cross order statistics");
    pass_need_kernel(launch_cross_order != nullptr, "cross-order");
    PassHold hold;
    pass_prepare(vs, n_vs, hold, "cross order statistics");
    const bool values = (outputs & FMHIP_CROSS_VALUES) != 0, indices = (outputs & FMHIP_CROSS_INDICES) != 0;
    const int n_out = fmhost::fm_cross_outputs(n_ranks, outputs);
    DevCrossOrderArgs a{};
    a.n = hold.n; a.n_vectors = (uint32_t)n_vs; a.n_values = values ? (uint32_t)n_ranks : 0u; a.n_indices = indices ? (uint32_t)n_ranks : 0u;
    for (int i = 0; i < fmhost::FM_CROSS_MAX_VECTORS; ++i) a.v[i] = hold.ptrs[(size_t)(i < n_vs ? i : n_vs - 1)];      // the kernel loads every word of its network
    PassOutputs made(this);
    std::vector<uint64_t> fresh((size_t)n_out);                          // in the caller's order: values of all selectors, then indices
    for (int o = 0; o < n_out; ++o) fresh[(size_t)o] = made.add(hold.n);
    // the launch wants them ordered by rank: position r owes [begin[r], begin[r + 1])
    uint32_t at = 0;
    for (int r = 0; r < n_vs; ++r) {
        a.value_begin[r] = values ? (uint8_t)at : 0; a.index_begin[r] = indices ? (uint8_t)at : 0;
        for (int j = 0; j < n_ranks; ++j) if (ranks[j] == r) {
            if (values) a.value_out[at] = fresh[(size_t)j];
            if (indices) a.index_out[at] = fresh[(size_t)((values ? n_ranks : 0) + j)];
            ++at;
        }
    }
    a.value_begin[n_vs] = (uint8_t)a.n_values; a.index_begin[n_vs] = (uint8_t)a.n_indices;
    hip_check(launch_cross_order(a, stream_), "launch fm_cross_order_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_vs + n_out);
    bytes_written_ += 4 * hold.n * n_out;
    made.commit(outs);
}

void Engine::cross_select(fmhip_vec index, const fmhip_vec* vs, int n_vs, fmhip_vec* out) {
    require_init();
    cross_order_check_select(index, vs, n_vs, out);
    std::vector<fmhip_vec> all; all.reserve((size_t)n_vs + 1);
    all.push_back(index);
    all.insert(all.end(), vs, vs + n_vs);
    pass_size(all.data(), (int)all.size(), "cross select");
    pass_need_kernel(launch_cross_select != nullptr, "cross-select");
    PassHold hold;
    pass_prepare(all.data(), (int)all.size(), hold, "cross select");
    DevCrossSelectArgs a{};
    a.n = hold.n; a.n_vectors = (uint32_t)n_vs; a.index = hold.ptrs[0];
    for (int i = 0; i < n_vs; ++i) a.v[i] = hold.ptrs[(size_t)i + 1];
    PassOutputs made(this);
    a.out = made.add(hold.n);
    hip_check(launch_cross_select(a, stream_), "launch fm_cross_select_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * 3;
    bytes_written_ += 4 * hold.n;
    made.commit(out);
}

} // namespace fm
