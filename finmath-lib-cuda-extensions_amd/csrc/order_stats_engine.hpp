// order_stats_engine.hpp — the engine's side of the device order statistics (kernels: kernels.hip, host loop:
// order_stats.hpp).  Part of runtime.cpp's translation unit (included at its end behind side_pass_engine.hpp, nowhere else).
//
// Replaces the reference's getQuantile / getQuantileExpectation / getHistogram (RandomVariableCuda.java:970-1091), which download the
// vector and sort it on the host: here a pass leaves a few hundred integers in pinned memory and the vector stays where it is.
//
// One function per kind of pass, each in the frame of side_pass_engine.hpp: one flush, the vectors' storage held, one launch for the whole
// batch, the wait under the engine lock; then the integers are copied out.
#include "runtime.hpp"
#include "kernels.h"
#include "order_stats.hpp"

#include <algorithm>
#include <cstring>

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_os.cpp has the stand-ins); the mirrors' host sort is a caller's choice
// (FMHIP_DEVICE_ORDER_STATS=0), never the engine's.
hipError_t launch_os_hist(const DevSelectArgs& a, const uint64_t* vecs, const uint32_t* slots, uint32_t batch, hipStream_t st) __attribute__((weak));
hipError_t launch_os_sum(const DevRankSumArgs& a, const uint64_t* vecs, const uint32_t* keys, uint32_t batch, hipStream_t st) __attribute__((weak));
hipError_t launch_os_count(const DevCountArgs& a, const double* bounds, hipStream_t st) __attribute__((weak));

static_assert(os::BINS == FM_OS_BINS && os::MAX_SLOTS == FM_OS_MAX_SLOTS, "order_stats.hpp and kernels.h describe the same passes");

int64_t Engine::os_size(const fmhip_vec* hs, int count) { return pass_size(hs, count, "order statistics"); }

// Pinned staging of a pass: [tables the launch reads (copied to the device in-stream)] [what the launch writes] [flag]
void Engine::os_hist_pass(const fmhip_vec* hs, int count, int S, const uint32_t* slots, uint32_t shift, uint64_t* hist_out) {
    if (S < 1 || S > FM_OS_MAX_SLOTS || shift > 24u || (shift & 7u) || !slots || !hist_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad radix-select pass");
    pass_need_kernel(launch_os_hist != nullptr, "radix-select");
    PassHold hold;
    pass_prepare(hs, count, hold, "order statistics");
    const size_t n_hist = (size_t)count * S * FM_OS_BINS, n_slots = (size_t)count * (1 + S);
    const size_t tab_bytes = pass_up256((size_t)count * 8) + pass_up256(n_slots * 4);
    const size_t counters_bytes = pass_up256(((size_t)count + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + pass_up256(n_hist * 4) + 64);
    pass_scratch(counters_bytes + n_hist * 4, tab_bytes);
    uint32_t* hist_host = reinterpret_cast<uint32_t*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + pass_up256(n_hist * 4));
    DevSelectArgs a{};
    a.c.counters = (uint32_t*)pass_zero_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.hist_dev = reinterpret_cast<uint32_t*>((char*)pass_zero_ + counters_bytes);
    a.hist_host = hist_host;
    a.S = (uint32_t)S; a.shift = shift;
    const uint64_t* dev_vecs = nullptr; const uint32_t* dev_slots = nullptr;
    if (count == 1) {
        a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0];
        std::memcpy(a.slots0, slots, n_slots * 4);
    } else {
        std::memcpy(stage, hold.ptrs.data(), (size_t)count * 8);
        std::memcpy(stage + pass_up256((size_t)count * 8), slots, n_slots * 4);
        hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(order statistics tables)");
        dev_vecs = (const uint64_t*)pass_other_; dev_slots = reinterpret_cast<const uint32_t*>((char*)pass_other_ + pass_up256((size_t)count * 8));
    }
    pass_launch(flag, a.c.done_flag, a.c.done_value, "radix-select pass", [&] { return launch_os_hist(a, dev_vecs, dev_slots, (uint32_t)count, stream_); });
    // (slots a vector does not use were not written: they stay zero in the caller's array)
    for (int k = 0; k < count; ++k) {
        const uint32_t ns = std::min<uint32_t>(slots[(size_t)k * (1 + S)], (uint32_t)S);
        const size_t base = (size_t)k * S * FM_OS_BINS;
        for (size_t i = 0; i < (size_t)ns * FM_OS_BINS; ++i) hist_out[base + i] = hist_host[base + i];
        for (size_t i = (size_t)ns * FM_OS_BINS; i < (size_t)S * FM_OS_BINS; ++i) hist_out[base + i] = 0;
    }
}

void Engine::os_sum_pass(const fmhip_vec* hs, int count, const uint32_t* keys, double* sums_out) {
    if (!keys || !sums_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad rank-sum pass");
    pass_need_kernel(launch_os_sum != nullptr, "rank-sum");
    PassHold hold;
    pass_prepare(hs, count, hold, "order statistics");
    const uint32_t blocks = os_sum_blocks(hold.n);
    const size_t tab_bytes = pass_up256((size_t)count * 8) + pass_up256((size_t)count * 8);
    const size_t counters_bytes = pass_up256(((size_t)count + 1) * 4);
    const size_t part_bytes = pass_up256((size_t)count * blocks * 8);
    char* stage = (char*)ensure_stage(tab_bytes + pass_up256((size_t)count * 8) + 64);
    pass_scratch(counters_bytes, tab_bytes + part_bytes);
    double* out_host = reinterpret_cast<double*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + pass_up256((size_t)count * 8));
    DevRankSumArgs a{};
    a.c.counters = (uint32_t*)pass_zero_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.partials = reinterpret_cast<double*>((char*)pass_other_ + tab_bytes);
    a.out_host = out_host;
    const uint64_t* dev_vecs = nullptr; const uint32_t* dev_keys = nullptr;
    if (count == 1) { a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0]; a.lo0 = keys[0]; a.hi0 = keys[1]; }
    else {
        std::memcpy(stage, hold.ptrs.data(), (size_t)count * 8);
        std::memcpy(stage + pass_up256((size_t)count * 8), keys, (size_t)count * 8);
        hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(order statistics tables)");
        dev_vecs = (const uint64_t*)pass_other_; dev_keys = reinterpret_cast<const uint32_t*>((char*)pass_other_ + pass_up256((size_t)count * 8));
    }
    pass_launch(flag, a.c.done_flag, a.c.done_value, "rank-sum pass", [&] { return launch_os_sum(a, dev_vecs, dev_keys, (uint32_t)count, stream_); });
    for (int k = 0; k < count; ++k) sums_out[k] = out_host[k];
}

void Engine::os_count_pass(fmhip_vec h, const double* ascending_bounds, int m, uint64_t* counts_out) {
    if (!ascending_bounds || !counts_out || m < 1 || m > FM_OS_MAX_BOUNDS) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad counting pass");
    for (int i = 0; i < m; ++i)
        if (ascending_bounds[i] != ascending_bounds[i] || (i > 0 && ascending_bounds[i] < ascending_bounds[i - 1])) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the bounds of a counting pass are ascending and not NaN");
    pass_need_kernel(launch_os_count != nullptr, "counting");
    PassHold hold;
    pass_prepare(&h, 1, hold, "order statistics");
    const size_t tab_bytes = pass_up256((size_t)m * 8);
    const size_t counters_bytes = pass_up256(2 * 4);
    const size_t counts_bytes = pass_up256(((size_t)m + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + counts_bytes + 64);
    pass_scratch(counters_bytes + counts_bytes, tab_bytes);
    uint32_t* counts_host = reinterpret_cast<uint32_t*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + counts_bytes);
    DevCountArgs a{};
    a.c.counters = (uint32_t*)pass_zero_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0];
    a.counts_dev = reinterpret_cast<uint32_t*>((char*)pass_zero_ + counters_bytes);
    a.counts_host = counts_host;
    a.m = (uint32_t)m;
    a.pow2 = 1u; while (a.pow2 * 2u <= (uint32_t)m) a.pow2 *= 2u;
    std::memcpy(stage, ascending_bounds, (size_t)m * 8);
    hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(bounds)");
    pass_launch(flag, a.c.done_flag, a.c.done_value, "counting pass", [&] { return launch_os_count(a, (const double*)pass_other_, stream_); });
    for (int i = 0; i <= m; ++i) counts_out[i] = counts_host[i];
}

} // namespace fm
