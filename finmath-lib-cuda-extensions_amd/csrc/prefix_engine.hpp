// prefix_engine.hpp — the engine's side of the device prefix sums (kernels: prefix_kernel.hip; definition, tree and chunk
// arithmetic: prefix_host.hpp).  Passes in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// Every statistic of the other passes weighs the paths equally.  A weighted sample — importance sampling, likelihood-ratio weights — needs
// the running sum of its weights along the sorted sample: a weighted quantile, a weighted expected shortfall, the whole expected-shortfall
// curve, the running average of an estimator.  The sort (§4.16) returns the weights reordered by the key; this is the prefix sum behind it,
// in fp64 like every other sum here, in a tree that is a function of n alone.
//
// Every call: the rows, bases and queries in the side-pass scratch, one launch that raises the flag and is waited for.
//
// One engine, one sample: a carry between the shards of a device list or the ranks of an expectation communicator is not built — such a
// call is FMHIP_ERR_UNSUPPORTED (abi.cpp, sharded.cpp and below), never the prefix sums of a part.
#include "runtime.hpp"
#include "prefix_kernel.h"

#include <cstring>

namespace fm {

// WEAK: see pass_need_kernel.
hipError_t launch_prefix_sums(const DevPrefixArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_prefix_queries(const DevPrefixArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void prefix_check_sums(fmhip_vec v, int mode, const fmhip_vec* out) {
    if (!v) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "prefix sums: of a vector");
    if (mode != FM_PREFIX_SUM && mode != FM_PREFIX_MEAN) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "prefix sums: mode " + std::to_string(mode) + " (FMHIP_PREFIX_SUM or FMHIP_PREFIX_MEAN)");
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "prefix sums: null pointer: out");
}
void prefix_check_queries(fmhip_vec v, const void* queries, int count, const void* sums_out, const char* what) {
    if (!v) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": of a vector");
    if (count < 1 || count > FM_PREFIX_MAX_QUERIES) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": " + std::to_string(count) + " queries (1 … " + std::to_string(FM_PREFIX_MAX_QUERIES) + ")");
    if (!queries || !sums_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": null pointer");
}
// fmhip_prefix_sums_host: the definition, with its complaints as engine errors
void prefix_sums_host_checked(const float* v, int64_t n, double* prefix_out) {
    pass_as_engine_error([&] { prefix_sums_host(v, n, prefix_out); });
}

// the size of the sample, or the refusals that need no look at the values: before anything is flushed or launched
int64_t Engine::prefix_size(fmhip_vec v, const char* what) {
    const int64_t n = pass_size(&v, 1, what);
    if (!prefix_size_ok(n)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + " of " + std::to_string(n) + " elements: at most 2^31 - 1");
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, std::string(what) + " with an expectation communicator of " + std::to_string(comm_world) + " ranks: a carry between the ranks is not built");
    pass_need_kernel(launch_prefix_sums != nullptr && launch_prefix_queries != nullptr && launch_sort_done != nullptr, "prefix-sum");
    return n;
}

void Engine::prefix_sums(fmhip_vec v, int mode, fmhip_vec* out, double* total_out) {
    require_init();
    prefix_check_sums(v, mode, out);
    const int64_t n = prefix_size(v, "prefix sums");
    PassHold hold;
    pass_prepare(&v, 1, hold, "prefix sums");
    PassOutputs outs(this);
    const uint64_t sums = outs.add(n);
    // pinned: [the total] [flag]
    char* stage = (char*)ensure_stage(256 + 64);
    pass_scratch(pass_up256(8), prefix_scratch_bytes(n, 0));
    double* total_host = reinterpret_cast<double*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + 256);
    DevPrefixArgs a{};
    a.n = (uint32_t)n; a.chunk_tiles = prefix_chunk_tiles(n); a.mode = (uint32_t)mode; a.kind = FM_PREFIX_QUERY_NONE;
    a.v = hold.ptrs[0]; a.out = sums; a.scratch = (char*)pass_other_; a.total_host = total_host;
    pass_launch_raising(flag, "prefix sums", [&] { return launch_prefix_sums(a, stream_); });
    algorithmic_bytes_ += 12 * n;                 // the totals read 4n, the apply reads 4n and writes 4n
    bytes_written_ += 4 * n;
    outs.commit(out);
    if (total_out) *total_out = *total_host;
}

// positions (at) or thresholds (search): one chain, the answers in the pinned block
void Engine::prefix_query_pass(fmhip_vec v, const int64_t* positions, const double* thresholds, int count, int relative, int64_t* positions_out, double* sums_out, double* total_out, const char* what) {
    require_init();
    prefix_check_queries(v, positions ? (const void*)positions : (const void*)thresholds, count, sums_out, what);
    if (thresholds && !positions_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": null pointer: positions_out");
    const int64_t n = prefix_size(v, what);
    if (positions)
        for (int j = 0; j < count; ++j)
            if (positions[j] < 0 || positions[j] >= n) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "position " + std::to_string(positions[j]) + " outside a vector of " + std::to_string(n));
    PassHold hold;
    pass_prepare(&v, 1, hold, what);
    // pinned: [queries (copied to the device in-stream)] [sums] [positions] [the total] [flag]
    const size_t q_bytes = prefix_queries_bytes(count);
    char* stage = (char*)ensure_stage(3 * q_bytes + 256 + 64);
    pass_scratch(pass_up256(8), prefix_scratch_bytes(n, count));
    uint64_t* q_host = reinterpret_cast<uint64_t*>(stage);
    double* sums_host = reinterpret_cast<double*>(stage + q_bytes);
    uint64_t* pos_host = reinterpret_cast<uint64_t*>(stage + 2 * q_bytes);
    double* total_host = reinterpret_cast<double*>(stage + 3 * q_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + 3 * q_bytes + 256);
    for (int j = 0; j < count; ++j) {
        if (positions) q_host[j] = (uint64_t)positions[j];
        else std::memcpy(&q_host[j], &thresholds[j], 8);
    }
    DevPrefixArgs a{};
    a.n = (uint32_t)n; a.chunk_tiles = prefix_chunk_tiles(n); a.kind = positions ? FM_PREFIX_QUERY_AT : FM_PREFIX_QUERY_SEARCH;
    a.count = (uint32_t)count; a.relative = relative != 0 ? 1u : 0u;
    a.v = hold.ptrs[0]; a.scratch = (char*)pass_other_; a.total_host = total_host; a.sums_host = sums_host; a.positions_host = pos_host;
    hip_check(hipMemcpyAsync(prefix_queries(a), stage, (size_t)count * 8, hipMemcpyHostToDevice, stream_), "H2D(prefix queries)");
    pass_launch_raising(flag, what, [&] { return launch_prefix_queries(a, stream_); });
    algorithmic_bytes_ += 4 * n;                  // the totals read the vector once; a query reads its chunk again
    for (int j = 0; j < count; ++j) sums_out[j] = sums_host[j];
    if (positions_out) for (int j = 0; j < count; ++j) positions_out[j] = (int64_t)pos_host[j];
    if (total_out) *total_out = *total_host;
}

void Engine::prefix_sums_at(fmhip_vec v, const int64_t* positions, int count, double* sums_out) {
    require_init();
    if (!positions) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "prefix sums at: null pointer");
    prefix_query_pass(v, positions, nullptr, count, 0, nullptr, sums_out, nullptr, "prefix sums at");
}

void Engine::prefix_search(fmhip_vec v, const double* thresholds, int count, int relative, int64_t* positions_out, double* sums_out, double* total_out) {
    require_init();
    if (!thresholds) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "prefix search: null pointer");
    prefix_query_pass(v, nullptr, thresholds, count, relative, positions_out, sums_out, total_out, "prefix search");
}

} // namespace fm
