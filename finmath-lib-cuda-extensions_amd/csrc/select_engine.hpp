// select_engine.hpp — the engine's side of the device selection (kernels: select_kernel.hip; definition and argument rules:
// select_host.hpp).  Producing passes in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// What no pass before could do: keep the paths on which a condition holds.  compress makes vectors of exactly `count` elements from the
// selected paths of up to 8 vectors (and their positions), expand puts such vectors back where they came from, gather reads by a caller's
// index — Longstaff–Schwartz on the in-the-money paths, conditional statistics, rare events, an index list carried to any number of vectors.
//
// TWO PHASES, and where this departs from the frame: a compress cannot allocate its outputs "before anything is launched", because their
// size is the count, and the count is on the device.  Phase 1 (counts → carry) leaves the count in pinned memory and raises the flag; the
// host waits, reads it, allocates outputs of exactly `count` elements through PassOutputs and launches phase 2 (the scatter, or the
// expansion) on the same scratch, with its own flag and wait.  One extra wait per call; a 1 % selection holds 1 % of the memory, not 100 %.
// The frame's guarantee stays: a refusal or a failed allocation at either stage leaves no vector, no byte and no written handle behind
// (phase 1 writes only the scratch and the pinned count).  count == 0: FMHIP_OK, every handle 0, nothing allocated — an empty vector is
// not a vector in this engine.  An expand finds a size mismatch of its values against the count behind phase 1, before it allocates.
//
// One engine, one sample: a device list of several shards or an expectation communicator of several ranks is FMHIP_ERR_UNSUPPORTED
// (sharded.cpp and below) — the shards' counts differ and an exchange between shards is not built.
#include "runtime.hpp"
#include "select_kernel.h"

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_select.cpp has the stand-ins).
hipError_t launch_select_count(const DevCompressArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_select_compress(const DevCompressArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_select_expand(const DevCompressArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_select_gather(const DevIndexGatherArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
static void select_check_vectors(const char* what, fmhip_vec first, const fmhip_vec* values, int n_values, const fmhip_vec* values_out) {
    if (!first) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": the " + (what[0] == 'g' ? "index" : "mask") + " is no vector");
    if (n_values > 0 && (!values || !values_out)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": values[" + std::to_string(i) + "] is no vector");
}
void select_check_compress(fmhip_vec mask, const fmhip_vec* values, int n_values, const fmhip_vec* values_out, const fmhip_vec* positions_out, const int64_t* count_out) {
    pass_as_engine_error([&] { select_check_values("compress", n_values, 0); });
    if (n_values == 0 && !positions_out && !count_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "compress: nothing asked for: no value vector, no positions_out and no count_out");
    select_check_vectors("compress", mask, values, n_values, values_out);
}
void select_check_expand(fmhip_vec mask, const fmhip_vec* values, int n_values, const fmhip_vec* values_out) {
    pass_as_engine_error([&] { select_check_values("expand", n_values, 1); });
    select_check_vectors("expand", mask, values, n_values, values_out);
}
void select_check_gather(fmhip_vec index, const fmhip_vec* values, int n_values, const fmhip_vec* values_out) {
    pass_as_engine_error([&] { select_check_values("gather", n_values, 1); });
    select_check_vectors("gather", index, values, n_values, values_out);
}
// … and with the size of the mask known
void select_check_mask_size(const char* what, int64_t n, bool want_positions) {
    pass_as_engine_error([&] { select_check_size(what, n, want_positions); });
}
// fmhip_compress_host, fmhip_expand_host, fmhip_gather_host: the definitions, with their complaints as engine errors
void compress_host_checked(const float* mask, int64_t n, const float* const* values, int n_values, float* const* values_out, int64_t* positions_out, int64_t* count_out) {
    pass_as_engine_error([&] { compress_host(mask, n, values, n_values, values_out, positions_out, count_out); });
}
void expand_host_checked(const float* mask, int64_t n, const float* const* values, int n_values, int64_t n_value_elements, double fill, float* const* values_out) {
    bool fits = true;
    pass_as_engine_error([&] { fits = expand_host(mask, n, values, n_values, n_value_elements, fill, values_out); });
    if (!fits) throw Error(FMHIP_ERR_SIZE_MISMATCH, "expand: the values have " + std::to_string(n_value_elements) + " elements, which is not the number of selected elements of the mask");
}
void gather_host_checked(const float* index, int64_t m, const float* const* values, int n_values, int64_t n, float* const* values_out) {
    pass_as_engine_error([&] { gather_host(index, m, values, n_values, n, values_out); });
}

// Phase 1 of a compress or an expand: the count of the mask, the chunk bases left in the scratch for phase 2.  a.mask is set.
int64_t Engine::select_count_phase(DevCompressArgs& a, int64_t n, const char* what) {
    char* stage = (char*)ensure_stage(256 + 64);                  // pinned: [the count] [flag]
    uint64_t* count_host = reinterpret_cast<uint64_t*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + 256);
    *count_host = ~uint64_t(0);
    pass_scratch(pass_up256(8), select_scratch_bytes(n));
    a.n = (uint32_t)n; a.chunk_tiles = prefix_chunk_tiles(n); a.scratch = (char*)pass_other_; a.count_host = count_host;
    pass_launch_raising(flag, what, [&] { return launch_select_count(a, stream_); });
    const uint64_t count = *count_host;
    if (count > (uint64_t)n) throw Error(FMHIP_ERR_HIP, std::string("the ") + what + " ended without delivering its count");
    algorithmic_bytes_ += 4 * n;
    return (int64_t)count;
}
// Phase 2: the launch on the scratch that phase 1 left, with a flag and a wait of its own.
template <class Launch>
void Engine::select_second_phase(const char* what, Launch launch) {
    char* stage = (char*)ensure_stage(256 + 64);
    pass_launch_raising(reinterpret_cast<volatile uint64_t*>(stage + 256), what, launch);
}

void Engine::compress(fmhip_vec mask, const fmhip_vec* values, int n_values, fmhip_vec* values_out, fmhip_vec* positions_out, int64_t* count_out) {
    require_init();
    select_check_compress(mask, values, n_values, values_out, positions_out, count_out);
    std::vector<fmhip_vec> sample{ mask };
    sample.insert(sample.end(), values, values + n_values);
    const int64_t n = pass_size(sample.data(), (int)sample.size(), "compress");
    select_check_mask_size("compress", n, positions_out != nullptr);
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, "compress with an expectation communicator of " + std::to_string(comm_world) + " ranks: an exchange between the ranks is not built");
    pass_need_kernel(launch_select_count != nullptr && launch_select_compress != nullptr && launch_sort_done != nullptr, "compress");
    PassHold hold;
    pass_prepare(sample.data(), (int)sample.size(), hold, "compress");
    DevCompressArgs a{};
    a.mask = hold.ptrs[0];
    const int64_t count = select_count_phase(a, n, "compress");
    const int64_t n_out = n_values + (positions_out ? 1 : 0);
    fmhip_vec ids[FM_SELECT_MAX_VALUES + 1] = {};
    if (count > 0 && n_out > 0) {
        PassOutputs made(this);
        a.count = (uint32_t)count; a.n_values = (uint32_t)n_values;
        for (int i = 0; i < n_values; ++i) { a.values[i] = hold.ptrs[(size_t)i + 1]; a.values_out[i] = made.add(count); }
        if (positions_out) a.positions_out = made.add(count);
        select_second_phase("compress", [&] { return launch_select_compress(a, stream_); });
        // the mask is read again, every value vector once; every output is written at its own size
        algorithmic_bytes_ += 4 * n + 4 * n * n_values + 4 * count * n_out;
        bytes_written_ += 4 * count * n_out;
        made.commit(ids);
    }
    for (int i = 0; i < n_values; ++i) values_out[i] = ids[i];
    if (positions_out) *positions_out = ids[n_values];
    if (count_out) *count_out = count;
}

void Engine::expand(fmhip_vec mask, const fmhip_vec* values, int n_values, double fill, fmhip_vec* values_out) {
    require_init();
    select_check_expand(mask, values, n_values, values_out);
    const int64_t n = pass_size(&mask, 1, "expand");
    const int64_t n_short = pass_size(values, n_values, "expand");
    select_check_mask_size("expand", n, false);
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, "expand with an expectation communicator of " + std::to_string(comm_world) + " ranks: an exchange between the ranks is not built");
    pass_need_kernel(launch_select_count != nullptr && launch_select_expand != nullptr && launch_sort_done != nullptr, "expand");
    PassHold hold, hold_values;
    pass_prepare(&mask, 1, hold, "expand");
    pass_prepare(values, n_values, hold_values, "expand");
    DevCompressArgs a{};
    a.mask = hold.ptrs[0];
    const int64_t count = select_count_phase(a, n, "expand");
    if (count != n_short) throw Error(FMHIP_ERR_SIZE_MISMATCH, "expand: the values have " + std::to_string(n_short) + " elements, the mask selects " + std::to_string(count));
    PassOutputs made(this);
    a.count = (uint32_t)count; a.n_values = (uint32_t)n_values; a.fill = (float)fill;
    for (int i = 0; i < n_values; ++i) { a.values[i] = hold_values.ptrs[(size_t)i]; a.values_out[i] = made.add(n); }
    select_second_phase("expand", [&] { return launch_select_expand(a, stream_); });
    algorithmic_bytes_ += 4 * n + (4 * count + 4 * n) * n_values;
    bytes_written_ += 4 * n * n_values;
    made.commit(values_out);
}

void Engine::gather(fmhip_vec index, const fmhip_vec* values, int n_values, fmhip_vec* values_out) {
    require_init();
    select_check_gather(index, values, n_values, values_out);
    const int64_t m = pass_size(&index, 1, "gather");
    const int64_t n = pass_size(values, n_values, "gather");
    select_check_mask_size("gather", m, false);
    select_check_mask_size("gather from a vector", n, false);
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, "gather with an expectation communicator of " + std::to_string(comm_world) + " ranks: an exchange between the ranks is not built");
    pass_need_kernel(launch_select_gather != nullptr && launch_sort_done != nullptr, "gather");
    PassHold hold, hold_values;
    pass_prepare(&index, 1, hold, "gather");
    pass_prepare(values, n_values, hold_values, "gather");
    PassOutputs made(this);
    DevIndexGatherArgs a{};
    a.n = (uint32_t)n; a.m = (uint32_t)m; a.n_values = (uint32_t)n_values; a.index = hold.ptrs[0];
    for (int i = 0; i < n_values; ++i) { a.values[i] = hold_values.ptrs[(size_t)i]; a.values_out[i] = made.add(m); }
    char* stage = (char*)ensure_stage(256 + 64);
    pass_launch_raising(reinterpret_cast<volatile uint64_t*>(stage + 256), "gather", [&] { return launch_select_gather(a, stream_); });
    algorithmic_bytes_ += 4 * m + 8 * m * n_values;
    bytes_written_ += 4 * m * n_values;
    made.commit(values_out);
}

} // namespace fm
