// order_stats_engine.hpp — the engine's side of the device order statistics (kernels: kernels.hip, host loop:
// order_stats.hpp).  Part of runtime.cpp's translation unit (included at its end, nowhere else): Engine member functions in a file of their
// own because runtime.cpp is long enough, and in that translation unit so that every build that lists the engine's sources — the library's,
// the sanitizer builds against the null device — has them without being told.
//
// Replaces the reference's getQuantile / getQuantileExpectation / getHistogram (RandomVariableCuda.java:970-1091), which download the
// vector and sort it on the host: here a pass leaves a few hundred integers in pinned memory and the vector stays where it is.
//
// One function per kind of pass.  Each: ends a step group, counts as a use of every vector (escape policy), computes what is pending or
// deferred below the batch in ONE flush, takes a reference on every vector's STORAGE and forgets the nodes — the wait that follows may not
// rely on a Node* (queued releases are not performed during it either: it polls the flag and falls back to the plain stream wait) —,
// launches once for the whole batch, waits under the engine lock as read() does, copies the integers out.  Shared storage (common rows)
// is only read.
#include "runtime.hpp"
#include "kernels.h"
#include "order_stats.hpp"

#include <algorithm>
#include <cstring>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace fm {

// The three launchers are WEAK references here: a host-only build of the engine whose stand-in for kernels.hip does not know these kernels
// (tests/nulldev/null_hip.cpp; tests/nulldev/null_os.cpp adds them) still links.  Calling one that is missing is an error — there is
// no fallback: the mirrors' host sort is a caller's choice (FMHIP_DEVICE_ORDER_STATS=0), never the engine's.
hipError_t launch_os_hist(const DevSelectArgs& a, const uint64_t* vecs, const uint32_t* slots, uint32_t batch, hipStream_t st) __attribute__((weak));
hipError_t launch_os_sum(const DevRankSumArgs& a, const uint64_t* vecs, const uint32_t* keys, uint32_t batch, hipStream_t st) __attribute__((weak));
hipError_t launch_os_count(const DevCountArgs& a, const double* bounds, hipStream_t st) __attribute__((weak));
static void os_need_kernel(bool present, const char* what) {
    if (!present) throw Error(FMHIP_ERR_UNSUPPORTED, std::string("this build of the engine has no ") + what + " kernel");
}

static_assert(os::BINS == FM_OS_BINS && os::MAX_SLOTS == FM_OS_MAX_SLOTS, "order_stats.hpp and kernels.h describe the same passes");

static size_t os_up256(size_t b) { return (b + 255) & ~size_t(255); }

struct Engine::OsHold {            // the storage of a batch, referenced for the duration of a pass
    Engine* e = nullptr;
    std::vector<Buffer*> held;
    std::vector<uint64_t> ptrs;
    int64_t n = 0;
    ~OsHold() { for (Buffer* b : held) e->buffer_unref(b); }
};

int64_t Engine::os_size(const fmhip_vec* hs, int count) {
    require_init();
    if (!hs || count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "order statistics of no vector");
    const int64_t n = node(hs[0])->n;
    for (int i = 1; i < count; ++i)
        if (node(hs[i])->n != n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "order statistics over vectors of different size");
    if (n <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "order statistics of an empty vector");
    return n;
}

void Engine::os_prepare(const fmhip_vec* hs, int count, OsHold& hold) {
    hold.e = this;
    hold.n = os_size(hs, count);
    if (count > 65535) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "more than 65535 vectors in one order-statistics call");
    end_step_group();
    std::vector<Node*> nds((size_t)count);
    bool pending = false, missing = false;
    for (int i = 0; i < count; ++i) {
        Node* nd = nds[(size_t)i] = node(hs[i]);
        if (nd->discarded && !nd->buf) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the value of this vector does not exist: it was given up (fmhip_vec_give_up_values: only its moments were taken), or lost in a launch that failed");
        touch(nd);
        missing |= !nd->buf;
        pending |= !nd->buf && !nd->deferred;
    }
    if (missing) {
        // one flush for the batch: everything pending runs as the batched launches it would have run as anyway; a handle keeps its node
        // alive through it (the caller holds every handle of the batch), so the nodes are looked at again, not remembered, behind it
        if (pending && count > 1) flush_all();
        for (int i = 0; i < count; ++i) { Node* nd = node(hs[i]); if (!nd->buf) materialize({ nd }); }
        for (int i = 0; i < count; ++i) nds[(size_t)i] = node(hs[i]);
    }
    hold.held.reserve((size_t)count); hold.ptrs.reserve((size_t)count);
    for (Node* nd : nds) {
        if (!nd->buf) throw Error(FMHIP_ERR_HIP, "a vector of the batch could not be computed");
        nd->buf->refs++;
        hold.held.push_back(nd->buf);
        hold.ptrs.push_back((uint64_t)(uintptr_t)nd->buf->ptr);
    }
}

void Engine::os_scratch(size_t zero_bytes, size_t other_bytes) {
    auto grow = [&](void*& p, size_t& cap, size_t need, bool zero) {
        if (need <= cap && !(zero && os_dirty_)) return;
        if (need > cap) {
            if (p) { hip_check(hipStreamSynchronize(stream_), "sync"); (void)hipFree(p); p = nullptr; cap = 0; }
            const size_t c = std::max(os_up256(need), size_t(1) << 16);
            hip_check(hipMalloc(&p, c), "hipMalloc(order statistics scratch)");
            cap = c;
        }
        if (zero) hip_check(hipMemsetAsync(p, 0, cap, stream_), "hipMemsetAsync(order statistics scratch)");
    };
    grow(os_zero_, os_zero_cap_, zero_bytes, true);
    os_dirty_ = false;
    grow(os_other_, os_other_cap_, other_bytes, false);
}

void Engine::os_release() {
    if (os_zero_) (void)hipFree(os_zero_);
    if (os_other_) (void)hipFree(os_other_);
    os_zero_ = os_other_ = nullptr; os_zero_cap_ = os_other_cap_ = 0; os_dirty_ = false;
}

void Engine::os_wait(volatile uint64_t* flag, uint64_t value) {
    const auto t0 = std::chrono::steady_clock::now();
    bool arrived = *flag == value;
    for (uint32_t spins = 1; !arrived; ++spins) {
#if defined(__x86_64__)
        _mm_pause();
#endif
        arrived = *flag == value;
        if (!arrived && (spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    if (!arrived) { hip_check(hipStreamSynchronize(stream_), "order statistics sync"); arrived = *flag == value; }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!arrived) throw Error(FMHIP_ERR_HIP, "an order-statistics launch ended without delivering its counts");
    os_dirty_ = false;
}

// Pinned staging of a pass: [tables the launch reads (copied to the device in-stream)] [what the launch writes] [flag]
void Engine::os_hist_pass(const fmhip_vec* hs, int count, int S, const uint32_t* slots, uint32_t shift, uint64_t* hist_out) {
    if (S < 1 || S > FM_OS_MAX_SLOTS || shift > 24u || (shift & 7u) || !slots || !hist_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad radix-select pass");
    os_need_kernel(launch_os_hist != nullptr, "radix-select");
    OsHold hold;
    os_prepare(hs, count, hold);
    const size_t n_hist = (size_t)count * S * FM_OS_BINS, n_slots = (size_t)count * (1 + S);
    const size_t tab_bytes = os_up256((size_t)count * 8) + os_up256(n_slots * 4);
    const size_t counters_bytes = os_up256(((size_t)count + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + os_up256(n_hist * 4) + 64);
    os_scratch(counters_bytes + n_hist * 4, tab_bytes);
    uint32_t* hist_host = reinterpret_cast<uint32_t*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + os_up256(n_hist * 4));
    DevSelectArgs a{};
    a.c.counters = (uint32_t*)os_zero_;
    a.c.done_flag = const_cast<uint64_t*>(flag); a.c.done_value = ++os_seq_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.hist_dev = reinterpret_cast<uint32_t*>((char*)os_zero_ + counters_bytes);
    a.hist_host = hist_host;
    a.S = (uint32_t)S; a.shift = shift;
    const uint64_t* dev_vecs = nullptr; const uint32_t* dev_slots = nullptr;
    if (count == 1) {
        a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0];
        std::memcpy(a.slots0, slots, n_slots * 4);
    } else {
        std::memcpy(stage, hold.ptrs.data(), (size_t)count * 8);
        std::memcpy(stage + os_up256((size_t)count * 8), slots, n_slots * 4);
        hip_check(hipMemcpyAsync(os_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(order statistics tables)");
        dev_vecs = (const uint64_t*)os_other_; dev_slots = reinterpret_cast<const uint32_t*>((char*)os_other_ + os_up256((size_t)count * 8));
    }
    *flag = 0;
    os_dirty_ = true;
    hip_check(launch_os_hist(a, dev_vecs, dev_slots, (uint32_t)count, stream_), "radix-select pass");
    ++n_launches_;
    os_wait(flag, a.c.done_value);
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
    os_need_kernel(launch_os_sum != nullptr, "rank-sum");
    OsHold hold;
    os_prepare(hs, count, hold);
    const uint32_t blocks = os_sum_blocks(hold.n);
    const size_t tab_bytes = os_up256((size_t)count * 8) + os_up256((size_t)count * 8);
    const size_t counters_bytes = os_up256(((size_t)count + 1) * 4);
    const size_t part_bytes = os_up256((size_t)count * blocks * 8);
    char* stage = (char*)ensure_stage(tab_bytes + os_up256((size_t)count * 8) + 64);
    os_scratch(counters_bytes, tab_bytes + part_bytes);
    double* out_host = reinterpret_cast<double*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + os_up256((size_t)count * 8));
    DevRankSumArgs a{};
    a.c.counters = (uint32_t*)os_zero_;
    a.c.done_flag = const_cast<uint64_t*>(flag); a.c.done_value = ++os_seq_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.partials = reinterpret_cast<double*>((char*)os_other_ + tab_bytes);
    a.out_host = out_host;
    const uint64_t* dev_vecs = nullptr; const uint32_t* dev_keys = nullptr;
    if (count == 1) { a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0]; a.lo0 = keys[0]; a.hi0 = keys[1]; }
    else {
        std::memcpy(stage, hold.ptrs.data(), (size_t)count * 8);
        std::memcpy(stage + os_up256((size_t)count * 8), keys, (size_t)count * 8);
        hip_check(hipMemcpyAsync(os_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(order statistics tables)");
        dev_vecs = (const uint64_t*)os_other_; dev_keys = reinterpret_cast<const uint32_t*>((char*)os_other_ + os_up256((size_t)count * 8));
    }
    *flag = 0;
    os_dirty_ = true;
    hip_check(launch_os_sum(a, dev_vecs, dev_keys, (uint32_t)count, stream_), "rank-sum pass");
    ++n_launches_;
    os_wait(flag, a.c.done_value);
    for (int k = 0; k < count; ++k) sums_out[k] = out_host[k];
}

void Engine::os_count_pass(fmhip_vec h, const double* ascending_bounds, int m, uint64_t* counts_out) {
    if (!ascending_bounds || !counts_out || m < 1 || m > FM_OS_MAX_BOUNDS) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad counting pass");
    for (int i = 0; i < m; ++i)
        if (ascending_bounds[i] != ascending_bounds[i] || (i > 0 && ascending_bounds[i] < ascending_bounds[i - 1])) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the bounds of a counting pass are ascending and not NaN");
    os_need_kernel(launch_os_count != nullptr, "counting");
    OsHold hold;
    os_prepare(&h, 1, hold);
    const size_t tab_bytes = os_up256((size_t)m * 8);
    const size_t counters_bytes = os_up256(2 * 4);
    const size_t counts_bytes = os_up256(((size_t)m + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + counts_bytes + 64);
    os_scratch(counters_bytes + counts_bytes, tab_bytes);
    uint32_t* counts_host = reinterpret_cast<uint32_t*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + counts_bytes);
    DevCountArgs a{};
    a.c.counters = (uint32_t*)os_zero_;
    a.c.done_flag = const_cast<uint64_t*>(flag); a.c.done_value = ++os_seq_;
    a.c.n = hold.n; a.c.tiles = (uint32_t)((hold.n + FM_OS_TILE - 1) / FM_OS_TILE);
    a.c.use_inline = 1; a.c.vec0 = hold.ptrs[0];
    a.counts_dev = reinterpret_cast<uint32_t*>((char*)os_zero_ + counters_bytes);
    a.counts_host = counts_host;
    a.m = (uint32_t)m;
    a.pow2 = 1u; while (a.pow2 * 2u <= (uint32_t)m) a.pow2 *= 2u;
    std::memcpy(stage, ascending_bounds, (size_t)m * 8);
    hip_check(hipMemcpyAsync(os_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(bounds)");
    *flag = 0;
    os_dirty_ = true;
    hip_check(launch_os_count(a, (const double*)os_other_, stream_), "counting pass");
    ++n_launches_;
    os_wait(flag, a.c.done_value);
    for (int i = 0; i <= m; ++i) counts_out[i] = counts_host[i];
}

} // namespace fm
