// runtime.cpp — see runtime.hpp.  Host-only C++; all device work goes through kernels.h.
#include "runtime.hpp"
#include "kernels.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <array>
#include <functional>
#include <map>
#include <sstream>
#include <thread>
#include <chrono>
#include <unordered_set>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace fm {
static std::atomic<uint64_t> g_te_malloc_ns{ 0 }, g_te_malloc_calls{ 0 }, g_te_init_ns{ 0 };     // FMHIP_TE_TRACE: where an engine's start goes

void EngineMutex::lock_slow(uint64_t me) {
    for (unsigned spins = 0;; ++spins) {
        uint64_t expected = 0;
        if (owner_.load(std::memory_order_relaxed) == 0 && owner_.compare_exchange_weak(expected, me, std::memory_order_acquire, std::memory_order_relaxed)) return;
        if (spins < 256) {
#if defined(__x86_64__)
            _mm_pause();
#endif
        } else if (spins < 320) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

void hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    const int code = (e == hipErrorOutOfMemory) ? FMHIP_ERR_OUT_OF_MEMORY : FMHIP_ERR_HIP;
    throw Error(code, std::string(what) + ": " + hipGetErrorString(e));
}

// Environment knobs: a switch that is on unless it is set to "0…", a size with a default.  Read once where they are used (static const).
static bool knob_on(const char* name) { const char* e = std::getenv(name); return !(e && e[0] == '0'); }
static size_t knob_size(const char* name, size_t dflt) { const char* e = std::getenv(name); return e ? (size_t)std::atoll(e) : dflt; }

// ---------------------------------------------------------------- opcode table

struct OpInfo { int n_vec; bool scalar; };
static OpInfo op_info(int opcode) {
    if (opcode >= FMHIP_OP_CAP_S && opcode <= FMHIP_OP_POW_S) return {1, true};
    if (opcode >= FMHIP_OP_SQUARED && opcode <= FMHIP_OP_ISNAN) return {1, false};
    if (opcode >= FMHIP_OP_CAP && opcode <= FMHIP_OP_DIV) return {2, false};
    if (opcode >= FMHIP_OP_ACCRUE && opcode <= FMHIP_OP_ADDPRODUCT_VS) return {2, true};
    if (opcode >= FMHIP_OP_ADDPRODUCT && opcode <= FMHIP_OP_CHOOSE) return {3, false};
    return {0, false};
}

// ---------------------------------------------------------------- pool

static size_t round_cap(size_t bytes) {
    size_t cap = (bytes + 255) & ~size_t(255);
    return cap ? cap : 256;
}

void* Pool::alloc(size_t bytes, size_t* cap_out) {
    const size_t cap = round_cap(bytes);
    *cap_out = cap;
    // test hook (tests/test_gpu_replicas.py): the N-th allocation of the process fails like a device that is out of memory
    static const long long FAIL_AT = [] { const char* e = std::getenv("FMHIP_TEST_FAIL_ALLOC_AT"); return e ? std::atoll(e) : 0ll; }();
    static std::atomic<long long> calls{ 0 };            // (several engines — thread engines, device lists — allocate side by side)
    if (FAIL_AT > 0 && ++calls == FAIL_AT) throw Error(FMHIP_ERR_OUT_OF_MEMORY, "device allocation failed (FMHIP_TEST_FAIL_ALLOC_AT)");
    std::vector<void*>& fl = free_[cap];
    if (!fl.empty()) {
        void* p = fl.back();
        fl.pop_back();
        hits++; cached -= (int64_t)cap; in_use += (int64_t)cap;
        return p;
    }
    // Miss.  Device allocations are expensive (≈ 100 µs each) and a Monte-Carlo state is thousands of equally sized vectors:
    // allocate SLABS of 1, 2, 4 … 64 blocks of this size class (≤ 1 GiB per slab) and hand the rest to the free list.
    const size_t grown = slab_blocks_[cap];
    size_t blocks = grown ? std::min<size_t>(grown * 2, 64) : 1;
    while (blocks > 1 && blocks * cap > (size_t(1) << 30)) blocks /= 2;
    void* base = nullptr;
    const auto tm0 = std::chrono::steady_clock::now();
    struct Tm { std::chrono::steady_clock::time_point t0; ~Tm() { g_te_malloc_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); ++g_te_malloc_calls; } } tm{ tm0 };
    // The pool never takes the LAST of the device: the HIP runtime itself allocates device memory while the process runs (code objects the
    // JIT tier loads, kernels loaded at their first launch, scratch, signals), and a caller whose handles die late — a garbage-collected
    // one — grows the pool until something fails.  With less than the headroom left a miss counts as out of memory (purge, then the error
    // the caller answers with a collection: RandomVariableCuda.java:311-335 does the same below a free-memory percentage).  Asked on a miss
    // only: a slab allocation costs ≈ 100 µs, the query a few.
    static const size_t HEADROOM = knob_size("FMHIP_POOL_HEADROOM_BYTES", (size_t(2) << 30));
    auto room_for = [&](size_t bytes) { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return true; } return fr >= bytes + HEADROOM; };
    hipError_t e = hipErrorOutOfMemory;
    if (blocks > 1 && !room_for(blocks * cap)) blocks = 1;
    if (room_for(blocks * cap)) {
        e = hipMalloc(&base, blocks * cap);
        if (e != hipSuccess && blocks > 1) { (void)hipGetLastError(); blocks = 1; e = hipMalloc(&base, cap); }
    }
    if (e != hipSuccess) {
        // The device is full.  (1) Cached slabs go back to the driver — as many as this allocation needs and a little more, not all of
        // them (the reference's last resort drops every cached buffer, RandomVariableCuda.java:340; here a caller whose collector had
        // just handed back 290 GB of vectors lost that whole cache to the next 40 KB allocation of an unusual size, and paid for it in
        // device allocations: 75 s instead of 6 for the calibration of lmm_hip --finmath-like --release-lag-bytes 268435456).
        (void)hipGetLastError();
        purge(cap + (size_t(256) << 20));
        blocks = 1;
        if (room_for(cap)) e = hipMalloc(&base, cap);
    }
    if (e != hipSuccess) {
        // (2) Nothing could be given back — slabs are freed whole, and every one of them has a live vector in it — but blocks of a LARGER
        // size class sit cached: one of them is carved into blocks of this class (a 40 KB buffer for a reduction's partials must not fail
        // while gigabytes are cached in 4 MB blocks).
        (void)hipGetLastError();
        if (void* p = borrow(cap)) { misses++; return p; }
        throw Error(FMHIP_ERR_OUT_OF_MEMORY, "device allocation of " + std::to_string(cap) + " bytes failed: " + hipGetErrorString(e) + " (the pool holds " + std::to_string(reserved >> 20) +
                    " MiB, " + std::to_string(in_use >> 20) + " MiB of them in live vectors; " + std::to_string(HEADROOM >> 20) + " MiB of the device are left to the HIP runtime)");
    }
    // (looked up again: purge() above drops the entries of size classes it has emptied — until round 5 a reference taken before the purge
    // was written through here, into a freed map node: heap corruption whenever an allocation of a rarely used size met a full device)
    slab_blocks_[cap] = blocks;
    slabs_.push_back({ base, cap, blocks, 0 });
    std::vector<void*>& fl2 = free_[cap];
    for (size_t i = blocks; i-- > 1;) { fl2.push_back((char*)base + i * cap); cached += (int64_t)cap; }
    misses++; reserved += (int64_t)(blocks * cap); in_use += (int64_t)cap;
    peak_reserved = std::max(peak_reserved, reserved);
    return base;
}

// A cached block of the smallest larger size class becomes a slab of this one (Slab::parent_cap); purge() hands it back when all its
// blocks are free again.
void* Pool::borrow(size_t cap) {
    size_t best = 0;
    for (const auto& kv : free_) if (kv.first > cap && !kv.second.empty() && (best == 0 || kv.first < best)) best = kv.first;
    if (!best) return nullptr;
    void* base = free_[best].back();
    free_[best].pop_back();
    const size_t blocks = best / cap;
    cached -= (int64_t)best;
    slabs_.push_back({ base, cap, blocks, best });
    std::vector<void*>& fl = free_[cap];
    for (size_t i = blocks; i-- > 1;) { fl.push_back((char*)base + i * cap); cached += (int64_t)cap; }
    in_use += (int64_t)cap;
    return base;
}

void Pool::release(void* p, size_t cap) {
    free_[cap].push_back(p);
    in_use -= (int64_t)cap; cached += (int64_t)cap;
}

// Slabs whose blocks are ALL back in the free list go back to the driver (a slab with one live vector stays) — all of them, or as many as
// it takes to give back `need` bytes.  Slabs that were carved out of a cached block (borrow) return that block to its own free list first.
void Pool::purge(size_t need) {
    std::unordered_map<size_t, std::unordered_set<void*>> free_set;
    for (auto& kv : free_) free_set[kv.first].insert(kv.second.begin(), kv.second.end());
    auto all_free = [&](const Slab& sl) {
        const std::unordered_set<void*>& fs = free_set[sl.cap];
        for (size_t i = 0; i < sl.blocks; ++i) if (!fs.count((char*)sl.base + i * sl.cap)) return false;
        return true;
    };
    std::vector<Slab> kept;
    for (const Slab& sl : slabs_) {                          // carved slabs first: their parents' slabs may become free by it
        if (!sl.parent_cap) { kept.push_back(sl); continue; }
        if (!all_free(sl)) { kept.push_back(sl); continue; }
        std::unordered_set<void*>& fs = free_set[sl.cap];
        for (size_t i = 0; i < sl.blocks; ++i) fs.erase((char*)sl.base + i * sl.cap);
        cached -= (int64_t)(sl.blocks * sl.cap);
        free_set[sl.parent_cap].insert(sl.base);
        cached += (int64_t)sl.parent_cap;
    }
    slabs_.swap(kept);
    kept.clear();
    size_t given_back = 0;
    for (size_t k = slabs_.size(); k-- > 0;) {                // youngest first: the old slabs hold the state a caller keeps
        const Slab& sl = slabs_[k];
        if (sl.parent_cap || given_back >= need || !all_free(sl)) { kept.push_back(sl); continue; }
        std::unordered_set<void*>& fs = free_set[sl.cap];
        for (size_t i = 0; i < sl.blocks; ++i) fs.erase((char*)sl.base + i * sl.cap);
        (void)hipFree(sl.base);
        reserved -= (int64_t)(sl.blocks * sl.cap); cached -= (int64_t)(sl.blocks * sl.cap);
        given_back += sl.blocks * sl.cap;
    }
    std::reverse(kept.begin(), kept.end());
    slabs_.swap(kept);
    free_.clear();
    for (auto& kv : free_set) if (!kv.second.empty()) free_[kv.first].assign(kv.second.begin(), kv.second.end());
    for (auto it = slab_blocks_.begin(); it != slab_blocks_.end();) {       // size classes without slabs start small again
        bool any = false;
        for (const Slab& sl : slabs_) any |= sl.cap == it->first && !sl.parent_cap;
        it = any ? std::next(it) : slab_blocks_.erase(it);
    }
}

// ---------------------------------------------------------------- engine lifecycle

// The engine of the calling thread: the process-wide one — or, on a worker thread of a device list (sharded.cpp: one engine per
// device shard, each driven by a thread of its own), that worker's.
static thread_local Engine* tls_engine = nullptr;
Engine& Engine::get() {
    if (tls_engine) { if (!tls_engine->retired.load(std::memory_order_acquire)) return *tls_engine; tls_engine = nullptr; }      // (a thread engine that fmhip_shutdown has retired)
    static Engine* e = new Engine();
    return *e;
}
Engine* Engine::create() { return new Engine(); }
void Engine::bind_thread(Engine* e) { tls_engine = e; }
bool Engine::thread_is_bound() { if (tls_engine && tls_engine->retired.load(std::memory_order_acquire)) tls_engine = nullptr; return tls_engine != nullptr; }

void Engine::require_init() const {
    if (!initialized_) throw Error(FMHIP_ERR_NOT_INITIALIZED, "fmhip_init has not been called");
    static thread_local int bound_device = -1;          // hipSetDevice is per thread; skip it on the hot path once bound
    if (bound_device != device_) { hip_check(hipSetDevice(device_), "hipSetDevice"); bound_device = device_; }
}

void fusion_max_weight_override(int v);      // FMHIP_FUSION_MAX_WEIGHT (experiments)
HostProfile g_host_profile;
void HostProfile::report() const {
    static const char* names[N_SLOTS] = { "call (record one method)", "release", "flush_all (total)", "  build_dag", "  run_dags (total)", "    launch (total)",
                                          "      kernel launch API", "      row table upload", "reduce / reduce_batch (total)",
                                          "  flush: roots + components", "  build_big (walk, schedule, sign)", "  run_big_group (total)",
                                          "graph_clone (total)" };
    std::fprintf(stderr, "[fmhip host profile]\n");
    for (int i = 0; i < N_SLOTS; ++i)
        std::fprintf(stderr, "  %-32s %10lld calls %9.3f s %9.2f us/call\n", names[i], count[i], seconds[i], count[i] ? seconds[i] / count[i] * 1e6 : 0.0);
}

void Engine::init(int device_index) {
    const auto ti0 = std::chrono::steady_clock::now();
    struct Ti { std::chrono::steady_clock::time_point t0; ~Ti() { g_te_init_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); } } ti{ ti0 };
    if (device_index < 0) {
        const char* e = std::getenv("FMHIP_DEVICE_INDEX");
        if (!e) e = std::getenv("LOCAL_RANK");
        device_index = e ? std::atoi(e) : 0;
    }
    int count = 0;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    if (count <= 0) throw Error(FMHIP_ERR_HIP, "no HIP device visible");
    if (device_index >= count) device_index = device_index % count;
    if (initialized_) {
        if (device_index != device_) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "already initialised on another device");
        return;
    }
    hip_check(hipSetDevice(device_index), "hipSetDevice");
    hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    ring_cap_ = size_t(32) << 20;                // row tables of rolled loops are ≈ 5 KB per row: room for hundreds of launches between wraps
    if (const char* e = std::getenv("FMHIP_RING_BYTES")) {      // tests shrink the ring so that a wrap costs a few launches, not thousands
        const long long v = std::atoll(e);
        if (v >= 4096) ring_cap_ = ((size_t)v + 255) & ~size_t(255);
    }
    hip_check(hipHostMalloc(&ring_host_, ring_cap_, hipHostMallocDefault), "hipHostMalloc(ring)");
    hip_check(hipMalloc(&ring_dev_, ring_cap_ + 256), "hipMalloc(ring)");
    hip_check(hipMalloc(&dump_dev_, FM_DUMP_BYTES), "hipMalloc(dump)");
    hip_check(hipHostMalloc((void**)&result_slots_, (size_t)RESULT_SLOTS * 128, hipHostMallocDefault), "hipHostMalloc(result slots)");
    ARENA_BYTES = size_t(16) << 20;
    if (const char* e = std::getenv("FMHIP_ARENA_BYTES")) { const long long v = std::atoll(e); if (v >= 1024) ARENA_BYTES = ((size_t)v + 31) & ~size_t(31); }      // tests: a wrap after a few dozen expectations
    hip_check(hipHostMalloc((void**)&moments_arena_, ARENA_BYTES, hipHostMallocDefault), "hipHostMalloc(moments arena)");
    arena_off_ = 0; arena_outstanding_.clear();
    free_slots_.clear();
    for (int i = RESULT_SLOTS; i-- > 0;) free_slots_.push_back(i);
    { const char* e = std::getenv("FMHIP_UNIT_WORKGROUPS"); unit_workgroups_ = e ? std::atoll(e) : 512; }
    hip_check(hipMalloc((void**)&counters_dev_, FM_COUNTER_PLANES * FM_COUNTER_PLANE * sizeof(uint32_t)), "hipMalloc(counters)");
    hip_check(hipMemsetAsync(counters_dev_, 0, FM_COUNTER_PLANES * FM_COUNTER_PLANE * sizeof(uint32_t), stream_), "hipMemset(counters)");
    hip_check(hipStreamSynchronize(stream_), "init sync");
    hip_check(preload_kernels(), "loading the device code");
    ring_off_ = 0;
    device_ = device_index;
    if (const char* e = std::getenv("FMHIP_JIT")) {
        const std::string v(e);
        if (v == "off" || v == "0") jit_mode = FMHIP_JIT_OFF;
        else if (v == "sync" || v == "2") jit_mode = FMHIP_JIT_SYNC;
        else if (v == "auto" || v == "1") jit_mode = FMHIP_JIT_AUTO;
    }
    if (!jit_shared_) jit_.start(device_index);              // (a thread engine uses the first engine's compiler and code objects)
    { static std::once_flag once; std::call_once(once, [] { g_host_profile.on = std::getenv("FMHIP_HOST_PROFILE") != nullptr; }); }      // (process-wide: several engines initialise side by side behind a device list)
    for (const char* name : { "FMHIP_BM_GROUP_STEPS", "FMHIP_GROUP_STEPS" })       // (the first: where round 2 had this, in BrownianMotionHip)
        if (const char* e = std::getenv(name)) { const int v = std::atoi(e); if (v >= 0) group_steps = v; }
    group_bm_id_ = 0; group_last_step_ = -1; group_steps_pending_ = 0; group_hold_ = false; group_last_by_bm_.clear();
    { static std::once_flag once; std::call_once(once, [] { if (const char* e = std::getenv("FMHIP_FUSION_MAX_WEIGHT")) { const int v = std::atoi(e); if (v > 0) fusion_max_weight_override(v); } }); }
    initialized_ = true;
}

void Engine::shutdown() {
    if (std::getenv("FMHIP_TE_TRACE")) std::fprintf(stderr, "[fmhip te] engine %d: so far in the process: hipMalloc of the pools %.1f ms in %llu calls, Engine::init %.1f ms\n", index_, g_te_malloc_ns.load() / 1e6, (unsigned long long)g_te_malloc_calls.load(), g_te_init_ns.load() / 1e6);
    if (!initialized_) return;
    drain_late();
    if (g_host_profile.on) g_host_profile.report();
    (void)hipSetDevice(device_);
    (void)hipStreamSynchronize(stream_);
    if (!jit_shared_) jit_.stop();      // joins the compiler thread, unloads the specialised kernels
    jit_shared_ = nullptr;
    nodes_.for_each([&](Node* nd) {     // leak-safe teardown: free storage of every live vector
        if (nd->buf) buffer_unref(nd->buf);     // back to the pool (blocks belong to slabs); purge() below frees the slabs
        delete nd;
    });
    nodes_.clear();
    for (auto& kv : replicas_) delete kv.second;
    replicas_.clear();
    pend_clear();
    for (Node* nd : node_pool_) delete nd;
    node_pool_.clear();
    for (auto& kv : programs_) if (--kv.second->refs == 0) delete kv.second;
    programs_.clear();
    for (auto& kv : plan_cache_) for (BigPlan::Seg& seg : kv.second.segs) { if (--seg.prog->refs == 0) delete seg.prog; delete seg.prog_red; }
    plan_cache_.clear();
    schedule_cache_.clear(); schedule_cache_bytes_ = 0; dag_policies_.clear(); policy_reset();
    for (auto& kv : program_cache_) if (--kv.second->refs == 0) delete kv.second;
    program_cache_.clear();
    pass_release();
    pool_.purge();
    pool_ = Pool();
    if (stage_) (void)hipHostFree(stage_);
    if (result_slots_) (void)hipHostFree(result_slots_);
    if (moments_arena_) (void)hipHostFree(moments_arena_);
    moments_arena_ = nullptr; arena_off_ = 0; arena_outstanding_.clear();
    for (auto& kv : tickets_) free_tickets_.push_back(kv.second);
    tickets_.clear();
    for (MomentsTicket& t : free_tickets_) { if (t.event) (void)hipEventDestroy(t.event); if (t.host) (void)hipHostFree(t.host); }
    free_tickets_.clear();
    result_slots_ = nullptr; free_slots_.clear();
    if (ring_host_) (void)hipHostFree(ring_host_);
    if (ring_dev_) (void)hipFree(ring_dev_);
    if (counters_dev_) (void)hipFree(counters_dev_);
    if (dump_dev_) (void)hipFree(dump_dev_);
    counters_dev_ = nullptr; dump_dev_ = nullptr;
    stage_ = ring_host_ = ring_dev_ = nullptr; stage_cap_ = ring_cap_ = ring_off_ = 0;
    (void)hipStreamDestroy(stream_);
    stream_ = nullptr;
    initialized_ = false;
    device_ = -1;
}

void Engine::synchronize() { require_init(); if (has_late()) drain_late(); hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize"); }

void Engine::device_info(char* name, int len, int* cus, int64_t* hbm) {
    require_init();
    hipDeviceProp_t prop;
    hip_check(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
    if (name && len > 0) {          // some boxes report an empty marketing name: fall back to the architecture string
        std::strncpy(name, prop.name[0] ? prop.name : prop.gcnArchName, (size_t)len - 1);
        name[len - 1] = 0;
    }
    if (cus) *cus = prop.multiProcessorCount;
    if (hbm) *hbm = (int64_t)prop.totalGlobalMem;
}

void* Engine::ensure_stage(size_t bytes) {
    if (bytes > stage_cap_) {
        if (stage_) { hip_check(hipStreamSynchronize(stream_), "sync"); (void)hipHostFree(stage_); stage_ = nullptr; stage_cap_ = 0; }
        size_t cap = std::max(bytes, size_t(1) << 20);
        hip_check(hipHostMalloc(&stage_, cap, hipHostMallocDefault), "hipHostMalloc(stage)");
        stage_cap_ = cap;
    }
    return stage_;
}

size_t Engine::ring_reserve(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (bytes > ring_cap_) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "batch too large for the row-table ring");
    if (ring_off_ + bytes > ring_cap_) {        // wrap: earlier tables may still be read by queued kernels
        wait_for_stream("hipStreamSynchronize(ring wrap)");
        ring_off_ = 0;
        ++ring_generation_;                     // device copies of earlier tables are about to be overwritten: nobody may reuse them
    }
    const size_t off = ring_off_;
    ring_off_ += bytes;
    return off;
}

// ---------------------------------------------------------------- buffers / nodes

Buffer* Engine::new_buffer(int64_t n_floats) {
    Buffer* b = new Buffer();
    size_t cap = 0;
    try { b->ptr = (float*)pool_.alloc((size_t)n_floats * 4, &cap); }
    catch (const Error& e) {
        // (out of memory with releases still queued: they are performed — their vectors go back to the pool — and the allocation is tried again)
        if (e.code != FMHIP_ERR_OUT_OF_MEMORY || !has_late()) { delete b; throw; }
        try { drain_late(); b->ptr = (float*)pool_.alloc((size_t)n_floats * 4, &cap); } catch (...) { delete b; throw; }
    }
    catch (...) { delete b; throw; }
    b->cap = cap; b->refs = 1;
    return b;
}

void Engine::buffer_unref(Buffer* b) {
    if (--b->refs > 0) return;
    if (b->foreign >= 0) {          // another engine's storage: whatever this stream still does with it comes before `done`; the owner's reference goes back later, outside this lock
        Foreign& f = foreign_[(size_t)b->foreign];
        hipEvent_t done = nullptr;
        if (hipEventCreateWithFlags(&done, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(done, stream_);
        foreign_done_.push_back({ f.owner, f.handle, done });
        import_of_.erase(f.handle);
        f.live = false;
        foreign_free_.push_back(b->foreign);
    } else if (b->parent) buffer_unref(b->parent);
    else pool_.release(b->ptr, b->cap);
    delete b;
}

void Engine::set_index(int i) {
    index_ = i;
    next_id_ = ((int64_t)i << OWNER_SHIFT) + 1;
    next_ticket_ = ((int64_t)i << OWNER_SHIFT) + 1;
}

Engine::Exported Engine::export_vector(fmhip_vec h, hipEvent_t ready) {
    require_init();
    Node* nd = node(h);
    touch(nd);
    if (!nd->buf) materialize({ nd });
    make_private(nd);               // (the importer aliases the storage by its address and is kept safe by a reference on THIS vector: storage shared with other vectors — common rows — could be given up by an in-place write here)
    nd->refs_ext++;
    hip_check(hipEventRecord(ready, stream_), "hipEventRecord(export)");
    Exported x;
    x.ptr = nd->buf->ptr; x.n = nd->n;
    if (nd->bm_id) { x.bm_id = ((uint32_t)(index_ + 1) << 24) | (nd->bm_id & 0xffffffu); x.bm_step = nd->bm_step; x.bm_steps = nd->bm_steps; }
    return x;
}

fmhip_vec Engine::import_vector(int owner, fmhip_vec owner_handle, const Exported& x, hipEvent_t ready) {
    require_init();
    hip_check(hipStreamWaitEvent(stream_, ready, 0), "hipStreamWaitEvent(import)");
    int32_t slot;
    if (!foreign_free_.empty()) { slot = foreign_free_.back(); foreign_free_.pop_back(); } else { slot = (int32_t)foreign_.size(); foreign_.push_back({}); }
    foreign_[(size_t)slot] = { owner, owner_handle, true };
    Buffer* b = new Buffer();
    b->ptr = x.ptr; b->cap = 0; b->refs = 1; b->foreign = slot;
    Node* nd = new_node(x.n);
    nd->buf = b;
    nd->moments_blocked = true;                                // (its moments, if anybody asks, are the owner's to keep)
    nd->bm_id = x.bm_id; nd->bm_step = x.bm_step; nd->bm_steps = x.bm_steps;
    import_of_[owner_handle] = nd;
    return nd->id;
}

fmhip_vec Engine::find_import(fmhip_vec foreign_handle) {
    auto it = import_of_.find(foreign_handle);
    if (it == import_of_.end()) return 0;
    Node* nd = it->second;                   // alive: it leaves the map when its storage goes (buffer_unref)
    if (++nd->refs_ext == 1) nodes_.put(nd->id, nd);          // kept by pending consumers only: a handle again
    return nd->id;
}

std::vector<Engine::ForeignDone> Engine::take_foreign_done() { std::vector<ForeignDone> out; out.swap(foreign_done_); return out; }

void Engine::release_exported(fmhip_vec h, hipEvent_t done) {
    require_init();
    if (done) (void)hipStreamWaitEvent(stream_, done, 0);
    release(h);
}

Node* Engine::new_node(int64_t n) {
    Node* nd;
    if (!node_pool_.empty()) { nd = node_pool_.back(); node_pool_.pop_back(); *nd = Node(); }      // recycled: no malloc on the hot path
    else nd = new Node();
    nd->id = next_id_++;
    nd->n = n;
    nd->refs_ext = 1;
    nodes_.put(nd->id, nd);
    return nd;
}

Node* Engine::node(fmhip_vec h) {
    if (owner_of(h) != index_) throw Error(FMHIP_ERR_INVALID_HANDLE, "vector handle " + std::to_string(h) + " belongs to another engine");
    Node* nd = nodes_.get(h);
    if (!nd) throw Error(FMHIP_ERR_INVALID_HANDLE, "invalid vector handle " + std::to_string(h));
    return nd;
}

void Engine::drop_expression(Node* nd) {
    for (int i = 0; i < nd->n_in; ++i) {
        Node* in = nd->in[i];
        nd->in[i] = nullptr;
        if (in) node_unref_int(in);
    }
    nd->n_in = 0; nd->opcode = 0; nd->weight = 0;
}

void Engine::node_unref_int(Node* nd) { nd->refs_int--; node_maybe_free(nd); }

void Engine::node_maybe_free(Node* nd) {
    if (nd->refs_ext > 0 || nd->refs_int > 0) return;
    if (nd->buf) buffer_unref(nd->buf);
    else { pend_erase(nd); drop_expression(nd); }
    static const size_t NODE_POOL_CAP = knob_size("FMHIP_NODE_POOL_CAP", (size_t)65536);      // (measured under a lagging collector: recycling ALL the nodes a burst of releases frees — random addresses — is no faster than fresh, consecutive ones)
    if (node_pool_.size() < NODE_POOL_CAP) node_pool_.push_back(nd); else delete nd;      // (a collector's burst frees hundreds of thousands at once: they are the next ones handed out, most recently touched first)
}

void Engine::retain(fmhip_vec h) { require_init(); node(h)->refs_ext++; }

void Engine::release(fmhip_vec h) {
    HostTimer timer(HostProfile::RELEASE);
    require_init();
    Node* nd = node(h);
    if (--nd->refs_ext == 0) { nodes_.erase(h); node_maybe_free(nd); }
}

void Engine::drain_late(size_t at_most) {
    const auto t_begin = std::chrono::steady_clock::now();
    struct Spent { Engine* e; std::chrono::steady_clock::time_point t0; ~Spent() { e->late_ns_ += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); } } spent{ this, t_begin };
    std::vector<fmhip_vec> batch;
    {
        std::lock_guard<std::mutex> lock(late_mu_);
        const size_t waiting = late_.size() - late_pos_;
        if (at_most >= waiting) { if (late_pos_ == 0) batch.swap(late_); else { batch.assign(late_.begin() + (std::ptrdiff_t)late_pos_, late_.end()); late_.clear(); } late_pos_ = 0; }
        else { batch.assign(late_.begin() + (std::ptrdiff_t)late_pos_, late_.begin() + (std::ptrdiff_t)(late_pos_ + at_most)); late_pos_ += at_most; }
        late_count_.store(late_.size() - late_pos_, std::memory_order_release);
    }
    if (!initialized_) return;
    (at_most == ~size_t(0) ? n_late_at_once_ : n_late_waiting_) += (int64_t)batch.size();
    // The nodes of handles that died a while ago are COLD, and performing a release touches several lines of several nodes: the node's
    // own three, its neighbours on the deferred list (unlinked), its operands (their counts drop; whatever only the recipe kept alive goes
    // with it).  Two stages of prefetching ahead of the work: the node itself 16 handles ahead, what it points to 8 ahead (by then it is there).
    static const size_t AHEAD = knob_size("FMHIP_DRAIN_PREFETCH", (size_t)8);
    std::vector<Node*> nds(batch.size());
    for (size_t i = 0; i < batch.size(); ++i) nds[i] = owner_of(batch[i]) == index_ ? nodes_.get(batch[i]) : nullptr;     // (a handle that is not one: nobody is left to tell)
    auto fetch = [](const void* p) { __builtin_prefetch(p, 1, 1); };
    for (size_t i = 0; i < batch.size(); ++i) {
        if (AHEAD) {
            if (i + 2 * AHEAD < batch.size()) if (const Node* far = nds[i + 2 * AHEAD]) { fetch(far); fetch((const char*)far + 64); fetch((const char*)far + 128); }
            if (i + AHEAD < batch.size()) if (const Node* near = nds[i + AHEAD]) {
                if (nodes_.get(batch[i + AHEAD]) == near && near->refs_ext == 1) {      // (still the handle's node: a handle released twice in one batch has lost it by now)                            // about to go: what its going touches
                    if (near->pend_prev) fetch(&near->pend_prev->pend_next);
                    if (near->pend_next) fetch(&near->pend_next->pend_prev);
                    if (!near->buf) for (int k = 0; k < near->n_in; ++k) if (near->in[k]) fetch(near->in[k]);
                }
            }
        }
        Node* nd = nds[i];
        if (!nd || nodes_.get(batch[i]) != nd) continue;             // (released twice in one batch: the second is not a handle any more)
        if (--nd->refs_ext == 0) { nodes_.erase(batch[i]); node_maybe_free(nd); }
    }
}

static void check_n(int64_t n) {
    if (n < 0 || n > (int64_t(1) << 31)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "invalid vector size " + std::to_string(n));
}

fmhip_vec Engine::create_uninitialized(int64_t n) {
    require_init(); check_n(n);
    Buffer* b = new_buffer(n);
    Node* nd = new_node(n);
    nd->buf = b;
    return nd->id;
}

fmhip_vec Engine::create_from_host(const void* src, bool is_double, int64_t n) {
    require_init(); check_n(n);
    if (n > 0 && !src) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "null host pointer");
    Buffer* b = new_buffer(n);
    try {
        const int64_t chunk = int64_t(16) << 20;            // floats per staging round (64 MiB)
        for (int64_t off = 0; off < n; off += chunk) {
            const int64_t m = std::min(chunk, n - off);
            float* st = (float*)ensure_stage((size_t)m * 4);
            if (is_double) {                                // (float)arrayOfDouble[i], RandomVariableCuda.java:768-774
                const double* s = (const double*)src + off;
                for (int64_t i = 0; i < m; ++i) st[i] = (float)s[i];
            } else std::memcpy(st, (const float*)src + off, (size_t)m * 4);
            hip_check(hipMemcpyAsync(b->ptr + off, st, (size_t)m * 4, hipMemcpyHostToDevice, stream_), "H2D");
            hip_check(hipStreamSynchronize(stream_), "H2D sync");
        }
    } catch (...) { buffer_unref(b); throw; }
    Node* nd = new_node(n);
    nd->buf = b;
    return nd->id;
}

fmhip_vec Engine::create_filled(int64_t n, float v) {
    require_init(); check_n(n);
    Buffer* b = new_buffer(n);
    if (n > 0) {
        hipError_t e = launch_fill(b->ptr, v, (int64_t)(round_cap((size_t)n * 4) / 4), stream_);
        if (e != hipSuccess) { buffer_unref(b); hip_check(e, "fill"); }
        n_launches_++;
    }
    Node* nd = new_node(n);
    nd->buf = b;
    return nd->id;
}

void Engine::read(fmhip_vec h, void* dst, bool as_double, int64_t n) {
    require_init();
    end_step_group();
    Node* nd = node(h);
    if (n != nd->n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "read of " + std::to_string(n) + " elements from a vector of " + std::to_string(nd->n));
    if (n > 0 && !dst) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "null host pointer");
    touch(nd);
    if (!nd->buf) materialize({nd});
    const int64_t chunk = int64_t(16) << 20;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        float* st = (float*)ensure_stage((size_t)m * 4);
        hip_check(hipMemcpyAsync(st, nd->buf->ptr + off, (size_t)m * 4, hipMemcpyDeviceToHost, stream_), "D2H");
        wait_for_stream("D2H sync");
        if (as_double) { double* d = (double*)dst + off; for (int64_t i = 0; i < m; ++i) d[i] = st[i]; }
        else std::memcpy((float*)dst + off, st, (size_t)m * 4);
    }
}

// Vectors are immutable but for two doors: a raw device pointer handed out, and fmhip_program_run_into.  Storage that several vectors share
// (rows of a batched launch that were identical and were computed once: run_peeled, merge_families) is copied before either opens.
void Engine::make_private(Node* nd) {
    Buffer* b = nd->buf;
    if (!b || b->refs <= 1 || b->parent || b->foreign >= 0) return;
    Buffer* own = new_buffer(nd->n);
    hipError_t e = hipMemcpyAsync(own->ptr, b->ptr, (size_t)nd->n * 4, hipMemcpyDeviceToDevice, stream_);
    if (e != hipSuccess) { buffer_unref(own); hip_check(e, "copy of a shared vector before it is written in place"); }
    nd->buf = own;
    buffer_unref(b);
}

void* Engine::device_ptr(fmhip_vec h) {
    require_init();
    end_step_group();
    Node* nd = node(h);
    touch(nd);
    if (!nd->buf) materialize({nd});
    // the caller may write through the pointer: whoever still reads this vector — pending expressions, recipes of deferred values — is computed first
    if (nd->refs_int > 0) { flush_all(); materialize_deferred(); }
    nd->has_moments = false; nd->moments_slot = nullptr; nd->moments_blocked = true;
    make_private(nd);
    return nd->buf->ptr;
}

// ---------------------------------------------------------------- program compiler (SSA → accumulator bytecode)
//
// Public opcode + "which operand is in the accumulator" → micro-op and the operand positions fetched from R.
struct UVariant { uint32_t uop; int r1_pos, r2_pos; };      // positions index {a,b,c}; -1 = unused
static bool variant_for(int opcode, int a_pos, UVariant* out) {
    auto set = [&](uint32_t u, int p1, int p2) { *out = { u, p1, p2 }; return true; };
    if (a_pos == 0) {
        switch (opcode) {
        case FMHIP_OP_CAP_S: return set(U_CAP_S, -1, -1);       case FMHIP_OP_FLOOR_S: return set(U_FLOOR_S, -1, -1);
        case FMHIP_OP_ADD_S: return set(U_ADD_S, -1, -1);       case FMHIP_OP_SUB_S: return set(U_SUB_S, -1, -1);
        case FMHIP_OP_BUS_S: return set(U_BUS_S, -1, -1);       case FMHIP_OP_MULT_S: return set(U_MULT_S, -1, -1);
        case FMHIP_OP_DIV_S: return set(U_DIV_S, -1, -1);       case FMHIP_OP_VID_S: return set(U_VID_S, -1, -1);
        case FMHIP_OP_POW_S: return set(U_POW_S, -1, -1);
        case FMHIP_OP_SQUARED: return set(U_SQUARED, -1, -1);   case FMHIP_OP_SQRT: return set(U_SQRT, -1, -1);
        case FMHIP_OP_EXP: return set(U_EXP, -1, -1);           case FMHIP_OP_LOG: return set(U_LOG, -1, -1);
        case FMHIP_OP_INVERT: return set(U_INVERT, -1, -1);     case FMHIP_OP_ABS: return set(U_ABS, -1, -1);
        case FMHIP_OP_SIN: return set(U_SIN, -1, -1);           case FMHIP_OP_COS: return set(U_COS, -1, -1);
        case FMHIP_OP_ISNAN: return set(U_ISNAN, -1, -1);
        case FMHIP_OP_CAP: return set(U_CAP, 1, -1);            case FMHIP_OP_FLOOR: return set(U_FLOOR, 1, -1);
        case FMHIP_OP_ADD: return set(U_ADD, 1, -1);            case FMHIP_OP_MULT: return set(U_MULT, 1, -1);
        case FMHIP_OP_SUB: return set(U_SUB, 1, -1);            case FMHIP_OP_DIV: return set(U_DIV, 1, -1);
        case FMHIP_OP_ACCRUE: return set(U_ACCRUE_A, 1, -1);    case FMHIP_OP_DISCOUNT: return set(U_DISCOUNT_A, 1, -1);
        case FMHIP_OP_ADDPRODUCT_VS: return set(U_ADDPRODUCT_VS_A, 1, -1);
        case FMHIP_OP_ADDPRODUCT: return set(U_ADDPRODUCT_A, 1, 2);
        case FMHIP_OP_ADDRATIO: return set(U_ADDRATIO_A, 1, 2); case FMHIP_OP_SUBRATIO: return set(U_SUBRATIO_A, 1, 2);
        case FMHIP_OP_CHOOSE: return set(U_CHOOSE_T, 1, 2);
        default: return false;
        }
    }
    if (a_pos == 1) {
        switch (opcode) {
        case FMHIP_OP_CAP: return set(U_CAP, 0, -1);            case FMHIP_OP_FLOOR: return set(U_FLOOR, 0, -1);   // min/max are symmetric
        case FMHIP_OP_ADD: return set(U_ADD, 0, -1);            case FMHIP_OP_MULT: return set(U_MULT, 0, -1);
        case FMHIP_OP_SUB: return set(U_BUS, 0, -1);            case FMHIP_OP_DIV: return set(U_VID, 0, -1);
        case FMHIP_OP_ACCRUE: return set(U_ACCRUE_B, 0, -1);    case FMHIP_OP_DISCOUNT: return set(U_DISCOUNT_B, 0, -1);
        case FMHIP_OP_ADDPRODUCT_VS: return set(U_ADDPRODUCT_VS_B, 0, -1);
        case FMHIP_OP_ADDPRODUCT: return set(U_ADDPRODUCT_B, 0, 2);
        case FMHIP_OP_CHOOSE: return set(U_CHOOSE_P, 0, 2);
        default: return false;
        }
    }
    if (a_pos == 2) {
        switch (opcode) {
        case FMHIP_OP_ADDPRODUCT: return set(U_ADDPRODUCT_B, 0, 1);     // a + c*b == a + b*c
        case FMHIP_OP_CHOOSE: return set(U_CHOOSE_N, 0, 1);
        default: return false;
        }
    }
    return false;
}

// … and the micro-op that runs: FMHIP_MATH_FAST takes the fast forms of exp and log (the interpreter's programs and the loop kernels alike)
static bool micro_op_for(int opcode, int a_pos, int math_mode, UVariant* out) {
    if (!variant_for(opcode, a_pos, out)) return false;
    if (math_mode == FMHIP_MATH_FAST) { if (out->uop == U_EXP) out->uop = U_EXP_FAST; else if (out->uop == U_LOG) out->uop = U_LOG_FAST; }
    return true;
}

// Position (0..2) at which value `v` can be consumed from the accumulator by `op`, or -1.
static int acc_position(const SsaOp& op, int n_vec, int v) {
    if (v < 0) return -1;
    const int ids[3] = { op.a, op.b, op.c };
    UVariant uv;
    for (int p = 0; p < n_vec; ++p) if (ids[p] == v && variant_for(op.opcode, p, &uv)) return p;
    return -1;
}

Program* Engine::compile(const std::vector<SsaOp>& ops, int n_in, const std::vector<int>& outs, const std::vector<int>& reds,
                         std::vector<float>* scalars_out, bool fixed_scalars)
{
    // Prefer the 8-elements-per-lane kernel (8 registers); fall back to 4 elements / 16 registers when the program
    // keeps more values alive.
    // fixed_scalars == false: the lazy front-end patches scalars per row, so no value-dependent rewrites are allowed
    bool library_math = false;          // pow / sin / cos live only in the 4-element kernel (see kernels.hip)
    for (const SsaOp& o : ops) library_math |= (o.opcode == FMHIP_OP_POW_S || o.opcode == FMHIP_OP_SIN || o.opcode == FMHIP_OP_COS);
    if (!library_math) {
        try { return compile_variant(ops, n_in, outs, reds, scalars_out, 1, fixed_scalars); }
        catch (const Error& e) { if (e.code != FMHIP_ERR_PROGRAM_LIMIT) throw; }
    }
    return compile_variant(ops, n_in, outs, reds, scalars_out, 0, fixed_scalars);
}

Program* Engine::compile_variant(const std::vector<SsaOp>& ops, int n_in, const std::vector<int>& outs, const std::vector<int>& reds,
                                 std::vector<float>* scalars_out, int variant, bool fixed_scalars)
{
    const int nreg_alloc = FM_VARIANT_NREG[variant] - 1;        // the last register is the "no store" dummy
    const unsigned no_store = (unsigned)nreg_alloc;
    const int n_ops = (int)ops.size();
    if (n_in < 0 || n_in > FM_MAX_IN || n_in > nreg_alloc) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many inputs for one launch");
    if (n_ops > FM_MAX_OPS) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many ops for one launch");
    if ((int)outs.size() > FM_MAX_OUT) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many outputs for one launch");
    if ((int)reds.size() > FM_MAX_RED) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many fused reductions for one launch");
    if (n_in == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "a program needs at least one input vector");
    const int n_val = n_in + n_ops;
    std::vector<int> n_vec(n_ops);
    for (int i = 0; i < n_ops; ++i) {
        const OpInfo inf = op_info(ops[i].opcode);
        if (inf.n_vec == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "unknown opcode " + std::to_string(ops[i].opcode));
        n_vec[i] = inf.n_vec;
        const int v[3] = { ops[i].a, ops[i].b, ops[i].c };
        for (int k = 0; k < inf.n_vec; ++k)
            if (v[k] < 0 || v[k] >= n_in + i) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "op " + std::to_string(i) + ": bad operand id");
    }
    for (int v : outs) if (v < 0 || v >= n_val) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad output value id");
    for (int v : reds) if (v < 0 || v >= n_val) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad reduce value id");

    // Pass 1: where does each op take its accumulator operand from, and which values must live in R?
    //   The result of op i-1 flows through the accumulator into op i when op i can consume it there;
    //   every other use of a value (and every program output / reduction) reads it from R.
    std::vector<int> apos(n_ops, -1);               // operand position served by the accumulator (-1: needs U_LDA of position 0)
    std::vector<int> last_r_use(n_val, -1);         // last op index reading the value from R (n_ops = program end)
    std::vector<char> stored(n_val, 0);
    for (int k = 0; k < n_in; ++k) stored[k] = 1;
    for (int i = 0; i < n_ops; ++i) {
        const int prev = (i > 0) ? n_in + i - 1 : -1;
        apos[i] = acc_position(ops[i], n_vec[i], prev);
        const int v[3] = { ops[i].a, ops[i].b, ops[i].c };
        for (int p = 0; p < n_vec[i]; ++p) {
            if (p == apos[i]) continue;
            stored[v[p]] = 1;
            last_r_use[v[p]] = i;
        }
    }
    for (int v : outs) { stored[v] = 1; last_r_use[v] = n_ops; }
    for (int v : reds) { stored[v] = 1; last_r_use[v] = n_ops; }

    // Pass 2: emit micro-ops with register allocation (a register is released after the value's last read from R).
    std::vector<int> reg_of(n_val, -1);
    std::vector<int> free_regs;
    for (int r = nreg_alloc - 1; r >= n_in; --r) free_regs.push_back(r);     // lowest register on top
    for (int k = 0; k < n_in; ++k) reg_of[k] = k;
    auto give_back = [&](int r) { free_regs.push_back(r); std::sort(free_regs.begin(), free_regs.end(), std::greater<int>()); };
    for (int k = 0; k < n_in; ++k) if (last_r_use[k] < 0) give_back(k);

    Program* p = new Program();
    p->n_in = n_in; p->n_out = (int)outs.size(); p->n_red = (int)reds.size(); p->n_ops = n_ops;
    std::vector<float> scal;
    int n_uops = 0;
    auto emit = [&](uint32_t word) {
        if (n_uops >= FM_MAX_OPS) { delete p; throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many micro-ops for one launch"); }
        p->proto.ops[n_uops++].w = word;
    };
    for (int i = 0; i < n_ops; ++i) {
        const int v[3] = { ops[i].a, ops[i].b, ops[i].c };
        int ap = apos[i];
        if (ap < 0) {                               // accumulator does not hold an operand: load position 0
            emit(fm_pack_op(U_LDA, (unsigned)reg_of[v[0]], 0, no_store, 0));
            ap = 0;
        }
        UVariant uv{};
        if (!micro_op_for(ops[i].opcode, ap, math_mode, &uv)) { delete p; throw Error(FMHIP_ERR_INVALID_ARGUMENT, "internal: no accumulator form"); }
        const unsigned r1 = uv.r1_pos >= 0 ? (unsigned)reg_of[v[uv.r1_pos]] : 0u;
        const unsigned r2 = uv.r2_pos >= 0 ? (unsigned)reg_of[v[uv.r2_pos]] : 0u;
        for (int q = 0; q < n_vec[i]; ++q) {        // values whose last read from R is this op free their register first
            bool dup = false;
            for (int j = 0; j < q; ++j) dup |= (v[j] == v[q]);
            if (!dup && last_r_use[v[q]] == i && reg_of[v[q]] >= 0) { give_back(reg_of[v[q]]); }
        }
        unsigned st = no_store;
        const int res = n_in + i;
        if (stored[res]) {
            if (free_regs.empty()) { delete p; throw Error(FMHIP_ERR_PROGRAM_LIMIT, "register budget of one launch exceeded"); }
            st = (unsigned)free_regs.back(); free_regs.pop_back();
            reg_of[res] = (int)st;
        }
        unsigned slot = 0;
        uint32_t uop = uv.uop;
        if (uop == U_LOG) p->proto.flags |= FM_ARGS_LOG_TABLE;
        if (op_info(ops[i].opcode).scalar) {
            if ((int)scal.size() >= FM_MAX_SCAL) { delete p; throw Error(FMHIP_ERR_PROGRAM_LIMIT, "too many scalar operands for one launch"); }
            slot = (unsigned)scal.size();
            float sv = (float)ops[i].scalar;        // "(float)value", RandomVariableCuda.java:521
            if (uop == U_DIV_S && fixed_scalars) {
                // a / (±2^k) == a * (±2^-k) bit for bit (both are the correctly rounded value of the same real number,
                // also for denormal results) as long as the reciprocal is itself a normal float: 1 multiply instead of
                // the 11-instruction IEEE division.  Only when the scalar is fixed at compile time (explicit programs).
                int ex = 0;
                const float mant = std::frexp(sv, &ex);
                if ((mant == 0.5f || mant == -0.5f) && ex > -124 && ex < 126) { uop = U_MULT_S; sv = 1.0f / sv; }
            }
            scal.push_back(sv);
        }
        emit(fm_pack_op(uop, r1, r2, st, slot));
    }
    for (size_t k = 0; k < outs.size(); ++k) p->proto.out_reg[k] = (uint32_t)reg_of[outs[k]];
    for (size_t k = 0; k < reds.size(); ++k) p->proto.red_reg[k] = (uint32_t)reg_of[reds[k]];
    if (scal.empty()) scal.push_back(0.0f);
    p->n_scal = (int)scal.size();
    p->proto.n_ops = (uint32_t)n_uops; p->proto.n_in = (uint32_t)n_in; p->proto.n_out = (uint32_t)outs.size();
    p->proto.n_red = (uint32_t)reds.size(); p->proto.n_scal = (uint32_t)p->n_scal;
    p->proto.variant = (uint32_t)variant;
    p->proto.row_words = (uint32_t)(n_in + (int)outs.size() + (int)reds.size() + (p->n_scal + 1) / 2);
    p->scalars = scal;
    if (scalars_out) *scalars_out = scal;
    return p;
}

// ---------------------------------------------------------------- launch

static const double JIT_HOT_WORK = [] { const char* e = std::getenv("FMHIP_JIT_HOT_WORK"); return e ? std::atof(e) : 2e10; }();    // element-ops on the interpreter before a lazy program is queued for specialisation

void Engine::launch(Program* p, int64_t n, const std::vector<RowSpec>& rows, fmhip_moments* host_moments, void* dev_moments)
{
    HostTimer timer(HostProfile::LAUNCH);
    const int batch = (int)rows.size();
    if (batch <= 0) return;
    if (batch > 65535) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "batch too large");
    const int n_red = p->n_red;
    {   // a row table that does not fit the pinned ring (FMHIP_RING_BYTES can be as small as 4 KB): as many rows per launch as fit
        const size_t row_bytes = (size_t)p->proto.row_words * 8;
        const size_t rows_fit = std::max<size_t>(1, (ring_cap_ - std::min<size_t>(ring_cap_, 256)) / row_bytes);
        if ((size_t)batch * p->proto.row_words > (size_t)FM_INLINE_WORDS && (size_t)batch > rows_fit) {
            for (size_t off = 0; off < (size_t)batch; off += rows_fit) {
                const size_t m = std::min(rows_fit, (size_t)batch - off);
                const std::vector<RowSpec> part(rows.begin() + (std::ptrdiff_t)off, rows.begin() + (std::ptrdiff_t)(off + m));
                launch(p, n, part, host_moments ? host_moments + off * n_red : nullptr, dev_moments ? (char*)dev_moments + off * n_red * 32 : nullptr);
            }
            return;
        }
    }
    if (n == 0) {       // nothing to compute; reductions of an empty vector as the twin's loops leave them (:288,:303,:325)
        if (host_moments) for (int i = 0; i < batch * n_red; ++i) host_moments[i] = { 0.0, 0.0, DBL_MAX, -DBL_MAX };
        if (dev_moments && n_red > 0) {
            std::vector<double> z((size_t)batch * n_red * 4);
            for (int i = 0; i < batch * n_red; ++i) { z[i * 4 + 0] = 0; z[i * 4 + 1] = 0; z[i * 4 + 2] = DBL_MAX; z[i * 4 + 3] = -DBL_MAX; }
            double* st = (double*)ensure_stage(z.size() * 8);
            std::memcpy(st, z.data(), z.size() * 8);
            hip_check(hipMemcpyAsync(dev_moments, st, z.size() * 8, hipMemcpyHostToDevice, stream_), "H2D");
            hip_check(hipStreamSynchronize(stream_), "sync");
        }
        return;
    }
    DevProgramArgs args = p->proto;
    // Tier selection.  Lazy programs are promoted once the interpreter has spent JIT_HOT_WORK element-ops on them
    // (≈10 ms of device time: a compilation costs ≈0.2 s of one background host core); explicit programs at creation.
    // A kernel that EXISTS (the user's code-object cache, the build-time pack) is used from the program's first launch: looked up once, on
    // this thread (two hashes of the generated source and a file).  Round 3's calibration ran 563 launches on the interpreter although
    // every one of those programs had its kernel in the pack.
    if (jit_mode == FMHIP_JIT_AUTO && !p->jit && !p->jit_probed) { p->jit_probed = true; p->jit = jit().request_cached(p->proto); }
    if (jit_mode != FMHIP_JIT_OFF && !p->jit) {
        p->interpreted_work += (double)n * batch * std::max(1, p->n_ops);       // (the stand-alone reduction has no ops: it counts as one)
        if (jit_mode == FMHIP_JIT_SYNC || p->interpreted_work >= JIT_HOT_WORK) p->jit = jit().request(p->proto, jit_mode == FMHIP_JIT_SYNC);
    } else if (jit_mode == FMHIP_JIT_SYNC && p->jit->state.load(std::memory_order_acquire) == JitSlot::QUEUED)
        p->jit = jit().request(p->proto, true);      // queued earlier in auto mode: finish it now
    const bool use_jit = jit_mode != FMHIP_JIT_OFF && p->jit && p->jit->state.load(std::memory_order_acquire) == JitSlot::READY;
    // the specialised kernel may process a different number of elements per lane and pass than the interpreter variant
    const int64_t elems_per_pass = (int64_t)FM_BLOCK * (use_jit ? p->jit->elems : FM_VARIANT_ELEMS[args.variant]);
    const int64_t tiles = (n + elems_per_pass - 1) / elems_per_pass;
    if (tiles > int64_t(0x7fffffff)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "vector too long");
    // Passes per workgroup.  A workgroup has a fixed cost (launch, log-table copy, for reductions the wave/LDS combine, the
    // partial write and the arrival counter) and, run back to back, kernels pay one workgroup lifetime of ramp-up and
    // tail: measured on the bench program (64 rows x 1M paths, benchmarks/jit_knobs.py) 2048 / 4096 / 8192 / 16384
    // elements per workgroup = 223 / 199 / 193 / 199 µs with fused reductions (181 / 179 / 177 / 186 µs without; there one
    // pass per workgroup is kept: on the LMM op stream, whose launches have 8 rows, 8192 gained 2 % and lost it again
    // together with the prefetch below).  With reductions the span must not depend on the batch: it fixes the order in
    // which a row's partial sums are added, and a value must not depend on how many other rows shared its launch.
    static const int64_t ELEMS_PER_BLOCK_ENV = [] { const char* e = std::getenv("FMHIP_ELEMS_PER_BLOCK"); const long long v = e ? std::atoll(e) : 0; return v >= 1024 ? (int64_t)v : (int64_t)0; }();
    // A program that evaluates log copies the 8 KB log table into LDS once per workgroup: one pass (2048 elements, 8 KB per
    // vector) per workgroup would double its L2 traffic (`log` alone: 88 → 95 µs), so it also gets ≈ 8192 elements per
    // workgroup — unless the launch is too small to fill the chip that way.
    const bool log_table = (args.flags & FM_ARGS_LOG_TABLE) != 0;
    const int64_t elems_per_block = ELEMS_PER_BLOCK_ENV ? ELEMS_PER_BLOCK_ENV : ((n_red > 0 || log_table) ? 8192 : 0);      // the variable: for benchmarks/jit_knobs.py
    int64_t passes_per_block = std::max<int64_t>(1, elems_per_block / elems_per_pass);
    if (n_red == 0) while (passes_per_block > 1 && ((tiles + passes_per_block - 1) / passes_per_block) * batch < 4096) passes_per_block /= 2;
    int64_t span_blocks = 1;
    if (n_red > 0) {
        // The reduction tree (fm_kernel_parts.hpp) is defined on units of 2048 elements and spans of four units — more for vectors of
        // more than 65536 spans, so that a row never has more workgroups than that.  A workgroup takes a whole span, or, where the
        // launch would leave most of the chip idle that way (one row of 1 M paths: 123 spans on 256 CUs), a single unit: four times
        // the workgroups, the same tree, the same moments.
        const int64_t unit_tiles = std::max<int64_t>(1, FM_UNIT_ELEMS / elems_per_pass);
        const int64_t units = (n + FM_UNIT_ELEMS - 1) / FM_UNIT_ELEMS;
        const int64_t span_units = ELEMS_PER_BLOCK_ENV ? std::max<int64_t>(1, ELEMS_PER_BLOCK_ENV / FM_UNIT_ELEMS) : std::max<int64_t>(FM_SPAN_UNITS, (units + 65535) / 65536);
        if (!ELEMS_PER_BLOCK_ENV && unit_launch(n, batch)) span_blocks = FM_SPAN_UNITS;
        passes_per_block = span_units / span_blocks * unit_tiles;
    } else if ((tiles + passes_per_block - 1) / passes_per_block > 65536) passes_per_block = (tiles + 65535) / 65536;
    const int64_t bpr = (tiles + passes_per_block - 1) / passes_per_block;
    args.block_tiles = (uint32_t)passes_per_block;
    args.span_blocks = (uint32_t)span_blocks;
    args.n = n;
    args.tiles_per_row = (uint32_t)tiles;
    const size_t rw = args.row_words;
    const size_t table_bytes = (size_t)batch * rw * 8;
    const uint64_t* dev_rows = nullptr;
    std::vector<uint64_t> table((size_t)batch * rw, 0);
    for (int b = 0; b < batch; ++b) {
        uint64_t* r = table.data() + (size_t)b * rw;
        const RowSpec& rs = rows[b];
        for (int k = 0; k < p->n_in; ++k) r[k] = (uint64_t)(uintptr_t)rs.in[k];
        for (int k = 0; k < p->n_out; ++k) r[p->n_in + k] = (uint64_t)(uintptr_t)rs.out[k];
        for (int k = 0; k < n_red; ++k) { const double s = rs.shifts ? rs.shifts[k] : 0.0; std::memcpy(&r[p->n_in + p->n_out + k], &s, 8); }
        float* sc = (float*)(r + p->n_in + p->n_out + n_red);
        const float* src = rs.scalars ? rs.scalars : p->scalars.data();
        for (int k = 0; k < p->n_scal; ++k) sc[k] = src[k];
    }
    // Small batches travel in the kernel arguments (≤ FM_INLINE_WORDS 8-byte words): the table upload is an in-stream copy
    // kernel of ≈ 5 µs (rocprofv3 on the LMM op stream: 1 579 of them, 6 % of the stream time, before this).
    if ((size_t)batch * rw <= (size_t)FM_INLINE_WORDS) { args.use_inline = 1; std::memcpy(args.inline_row, table.data(), (size_t)batch * rw * 8); }
    else {
        args.use_inline = 0;
        // A loop that runs the same program over the same vectors (run_into: time stepping with fixed buffers, bench.py)
        // re-creates the same table every time: if the copy uploaded last time is still in the ring, use it again and
        // save the in-stream H2D copy (≈ 5-8 µs of stream time per launch).
        if (p->last_dev_rows && p->last_ring_generation == ring_generation_ && p->last_table == table) dev_rows = p->last_dev_rows;
        else {
            HostTimer t2(HostProfile::ROW_UPLOAD);
            const size_t ring_off = ring_reserve(table_bytes);          // may wrap (and bump the generation)
            std::memcpy((char*)ring_host_ + ring_off, table.data(), table_bytes);
            hip_check(hipMemcpyAsync((char*)ring_dev_ + ring_off, (char*)ring_host_ + ring_off, table_bytes, hipMemcpyHostToDevice, stream_), "row table H2D");
            dev_rows = (const uint64_t*)((char*)ring_dev_ + ring_off);
            p->last_table.swap(table);
            p->last_dev_rows = dev_rows;
            p->last_ring_generation = ring_generation_;
        }
    }

    RedLaunch red;
    if (n_red > 0) red_begin(red, batch, n_red, (size_t)bpr, host_moments, dev_moments);
    args.results = (double*)red.results;
    args.counters = counters_dev_;
    args.done_flag = const_cast<uint64_t*>(red.poll_flag); args.done_value = red.done_value;
    void* const partials = red.partials;
    try {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        if (profiling_) {
            hip_check(hipEventCreate(&ev0), "hipEventCreate"); hip_check(hipEventCreate(&ev1), "hipEventCreate");
            hip_check(hipEventRecord(ev0, stream_), "hipEventRecord");
        }
        HostTimer t3(HostProfile::LAUNCH_API);
        const bool used_jit = use_jit;
        if (use_jit) {
            const uint64_t* rows_arg = dev_rows; double* partials_arg = (double*)partials;
            void* params[] = { &args, &rows_arg, &partials_arg };
            hip_check(hipModuleLaunchKernel(args.use_inline ? p->jit->fn_inline : p->jit->fn_table, (unsigned)bpr, (unsigned)batch, 1, FM_BLOCK, 1, 1,
                                            0, stream_, params, nullptr), "launch specialised kernel");
            n_jit_launches_++;
        } else
            hip_check(launch_program(args, dev_rows, (double*)partials, (uint32_t)bpr, (uint32_t)batch, stream_), "launch fm_program_kernel");
        if (profiling_) { hip_check(hipEventRecord(ev1, stream_), "hipEventRecord"); profile_events_.push_back({ ev0, ev1 });
                          profile_tags_.push_back({ p->n_ops, p->n_in, p->n_out, n_red, batch, used_jit ? 1 : 0, n }); }
        n_launches_++; n_ops_executed_ += (int64_t)p->n_ops * batch;
        algorithmic_bytes_ += 4 * n * (int64_t)(p->n_in + p->n_out) * batch;
        bytes_written_ += 4 * n * (int64_t)p->n_out * batch;
        if (!used_jit) n_interpreter_launches_++;
        if (n_red > 0) {                     // the final combine ran inside the same launch (last workgroup of each row)
            if (defer_red_ && !defer_red_->pending && host_moments && red.on_host) {
                red.pending = true; red.batch = batch; red.n_red = n_red; red.host = host_moments;
                *defer_red_ = red;              // reduce() waits and releases
                return;
            }
            red_wait(red, batch, n_red, host_moments);
        }
    } catch (...) { red_release(red); throw; }
    red_release(red);
}

// Waits for everything queued on the stream — and, while it waits, performs releases that other threads have queued (drain_late): the
// device is asked whether it is done between portions instead of being slept on.
void Engine::wait_for_stream(const char* what)
{
    if (has_late()) {
        for (;;) {
            const hipError_t q = hipStreamQuery(stream_);
            if (q == hipSuccess) return;
            if (q != hipErrorNotReady) hip_check(q, what);
            (void)hipGetLastError();
            if (!has_late()) break;
            drain_late(late_portion());
        }
    }
    hip_check(hipStreamSynchronize(stream_), what);
}

// A launch with fused reductions over `batch` rows of n elements gives every workgroup one unit of the reduction tree (instead of a span
// of four) when it has few spans in all: such a launch has as many workgroups as one without reductions, so a chain over many vectors
// need not fear it.
bool Engine::unit_launch(int64_t n, int64_t batch) const
{
    const int64_t units = (n + FM_UNIT_ELEMS - 1) / FM_UNIT_ELEMS, spans = (units + FM_SPAN_UNITS - 1) / FM_SPAN_UNITS;
    return spans <= 65536 && spans * batch <= unit_workgroups_;
}

// ---------------------------------------------------------------- lazy front-end

static int FUSION_MAX_WEIGHT = 40;    // pending ops below one node before it is executed on its own accord.  Measured on the LMM
                                       // calibration (same box, FMHIP_FUSION_MAX_WEIGHT=40 vs 1000): 6.3 s vs 6.8-7.6 s although the
                                       // larger value needs 3x fewer launches — executing early overlaps device work with the
                                       // recording of the next methods, and that path is host-bound

void fusion_max_weight_override(int v) { FUSION_MAX_WEIGHT = v; }
static const size_t SPECULATE_PENDING = knob_size("FMHIP_SPECULATE_PENDING", (size_t)2000);   // operations recorded since the last time step; 0 = off.  5000 until the second half of round 5, when the device was what the hint-free calibration waited for; with the
                                                         // swaptions of an exercise date merged (merge_families) it is the host, and what counts is how little is left to run when the caller asks for its first expectation: 1500 / 2000 / 2500 / 3000 / 4000 / 5000
                                                         // methods: 3.48 / 3.37–3.45 / 3.46–3.55 / 3.56 / 3.63 / 3.66–3.70 s on one box (profiles/round05b_merged_chains.txt)
static const size_t SPECULATE_IDLE_MIN = knob_size("FMHIP_SPECULATE_IDLE_MIN", (size_t)0);   // 0 (default) = the device's idleness is not looked at.  Measured, lmm_hip --finmath-like at 1 M paths on one box: off 4.68 s; 512 / 1024 / 2048 / 4096: 5.26 / 4.89 / 4.96 / 4.90 s —
                                                         // chains cut wherever the device happens to run dry are shapes that never repeat (70 kernels compiled instead of 38, 4–12 k launches on the interpreter)
static const size_t FUSION_SOFT_CAP = 32768;     // pending operations at which a SOFT hold (fmhip_fusion_hold(2)) executes everything
// Experiment knob (off): execute everything once this many operations are pending anywhere, instead of the per-handle weight rule.
// On the hint-free LMM calibration (lmm_hip --finmath-like) 1000 … 16000 gave 15-18 ms per evaluation against 22.8 with the
// weight rule and 12.5 with BrownianMotionHip's time-step grouping: cut points that do not coincide with time steps give graph
// shapes that never repeat, so every flush plans from scratch and nothing rolls.
static size_t FUSION_MAX_PENDING = knob_size("FMHIP_FUSION_MAX_PENDING", (size_t)0);   // 0 = off

fmhip_vec Engine::call(int opcode, int n_in, const fmhip_vec* in, double scalar, bool has_scalar) {
    HostTimer timer(HostProfile::CALL);
    require_init();
    const OpInfo inf = op_info(opcode);
    if (inf.n_vec == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "unknown opcode " + std::to_string(opcode));
    if (inf.n_vec != n_in || inf.scalar != has_scalar)
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "opcode " + std::to_string(opcode) + " does not match this call shape");
    Node* ins[3] = { nullptr, nullptr, nullptr };
    for (int i = 0; i < n_in; ++i) {
        ins[i] = node(in[i]);
        if (ins[i]->discarded && !ins[i]->buf) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the value of an operand does not exist: it was given up (fmhip_vec_give_up_values), or lost in a launch that failed");
    }
    if (!replicas_.empty())                                     // an operation on the root of a copy that exists as a description only: the copy becomes an expression first
        for (int i = 0; i < n_in; ++i) if (!ins[i]->buf && ins[i]->rep_copy) if (ReplicaGroup* g = replica_of(ins[i])) expand_replicas(g);
    for (int i = 1; i < n_in; ++i)
        if (ins[i]->n != ins[0]->n)
            throw Error(FMHIP_ERR_SIZE_MISMATCH, "operand sizes differ: " + std::to_string(ins[0]->n) + " vs " + std::to_string(ins[i]->n));
    // the caller uses these handles again: what the escape policy has learnt about their positions; a value that was left unstored is
    // computed from its recipe now and stored (once)
    for (int i = 0; i < n_in; ++i) if (ins[i]->watch || ins[i]->deferred) demand(ins[i]);
    if (fusion && group_steps > 0 && fusion_hold == 0)         // a caller's own hold (or eager mode) leaves nothing to group on its behalf
        for (int i = 0; i < n_in; ++i)
            if (ins[i]->bm_id && (ins[i]->bm_step != group_last_step_ || ins[i]->bm_id != group_bm_id_)) step_boundary(ins[i]);
    Node* nd = new_node(ins[0]->n);
    nd->opcode = opcode; nd->n_in = n_in; nd->scalar = scalar;
    int w = 1;
    for (int i = 0; i < n_in; ++i) { nd->in[i] = ins[i]; ins[i]->refs_int++; w += ins[i]->buf ? 0 : ins[i]->weight; }
    nd->weight = w;
    pend_insert(nd);
    ++ops_since_boundary_;
    const bool held = fusion_hold != 0 || group_hold_;
    if (!fusion || (w > FUSION_MAX_WEIGHT && !held)) {
        try { materialize({nd}); }
        catch (...) { nd->refs_ext = 0; nodes_.erase(nd->id); node_maybe_free(nd); throw; }
    } else if (SPECULATE_PENDING && group_hold_ && fusion_hold == 0 &&
               (ops_since_boundary_ > SPECULATE_PENDING ||
                // … or much sooner when the device has NOTHING to do (asked every 128 methods, from SPECULATE_IDLE_MIN pending ones on): the
                // caller records the payoffs behind a simulation whose launches have drained — whatever is complete enough to run keeps the
                // device busy while the recording goes on.  The count above is the cut for a device that is still busy: larger launches.
                (SPECULATE_IDLE_MIN && ops_since_boundary_ >= SPECULATE_IDLE_MIN && (ops_since_boundary_ & 127) == 0 && hipStreamQuery(stream_) == hipSuccess))) {
        // The engine's own hold (time steps being grouped), no new time step for thousands of operations, and a caller that keeps
        // recording without asking for anything (the payoffs of its products, behind the simulation): what is pending runs now, without
        // waiting for it, and the launches take the moments of their roots along — when the caller comes to ask for expectations
        // (Engine::reduce), the device has been at work while the caller was recording.
        const fmhip_vec id = nd->id;
        ops_since_boundary_ = 0;
        MomentsAlong along(this, true);
        try { flush_all(); }
        catch (...) {
            if (nodes_.get(id) == nd) { nd->refs_ext = 0; nodes_.erase(id); node_maybe_free(nd); }
            throw;
        }
    } else if ((FUSION_MAX_PENDING && !held && n_pending_ > FUSION_MAX_PENDING) || ((fusion_hold == 2 || (group_hold_ && fusion_hold == 0)) && n_pending_ > FUSION_SOFT_CAP)) {
        const fmhip_vec id = nd->id;
        try { flush_all(); }
        catch (...) {                       // the caller never receives this handle: take the node (and whatever still hangs below it) back
            if (nodes_.get(id) == nd) { nd->refs_ext = 0; nodes_.erase(id); node_maybe_free(nd); }
            throw;
        }
        return id;
    }
    return nd->id;
}

// The first use of a Brownian increment with a new time index: a time step of the caller's discretisation scheme begins (what
// BrownianMotionHip did for itself in round 2, now for every caller of fmhip_bm_generate's vectors, whatever class wraps them).
// Index 0, or an index below the last one, starts a new simulation; the last index ends the grouping — what follows the
// simulation is not the scheme's to group.
void Engine::step_boundary(const Node* inc) {
    // Per generation: the time index it was last used with.  A generation that goes BACK (or starts at index 0) begins a new simulation;
    // another generation at the time index just seen is the second Brownian motion of a hybrid model inside the same time step — not a
    // boundary; and two simulations that take turns (two threads, two models) do not reset each other's count any more: until round 4 the
    // state was one (generation, index) pair, every change of generation was a "restart", and such callers never reached a flush of
    // their own (results unaffected; the work ran at the 32768-operation cap instead, in shapes that never repeat).
    if (group_last_by_bm_.size() > 64) group_last_by_bm_.clear();
    auto known = group_last_by_bm_.find(inc->bm_id);
    const int32_t last_of_this = known == group_last_by_bm_.end() ? -1 : known->second;
    if (inc->bm_step == last_of_this) { group_bm_id_ = inc->bm_id; group_last_step_ = inc->bm_step; return; }      // this generation's current time step again (the generations of a hybrid model take turns)
    const bool restart = inc->bm_step == 0 || inc->bm_step < last_of_this;
    const bool same_time_index = !restart && inc->bm_id != group_bm_id_ && inc->bm_step == group_last_step_;
    group_last_by_bm_[inc->bm_id] = inc->bm_step;
    group_bm_id_ = inc->bm_id; group_last_step_ = inc->bm_step;
    if (same_time_index) return;
    ops_since_boundary_ = 0;
    if (restart) group_steps_pending_ = 0;
    if (group_steps_pending_ == 0) group_hold_ = true;
    if (++group_steps_pending_ > group_steps) { flush_all(); group_steps_pending_ = 1; }
    if (inc->bm_step == inc->bm_steps - 1) { group_steps_pending_ = 0; group_last_step_ = -1; group_bm_id_ = 0; group_hold_ = false; group_last_by_bm_.erase(inc->bm_id); }
}

// ---------------------------------------------------------------- replication of pending graphs (fmhip_graph_clone)

void Engine::collect_pending(const fmhip_vec* roots, int n_roots, std::vector<Node*>& graph) {
    if (n_roots <= 0 || !roots) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "no roots");
    if (!replicas_.empty())                                     // the root of a copy that exists as a description only: it becomes an expression first
        for (int r = 0; r < n_roots; ++r) { Node* root = node(roots[r]); if (!root->buf && root->rep_copy) if (ReplicaGroup* g = replica_of(root)) expand_replicas(g); }
    const uint64_t ep = ++epoch_;
    std::vector<Node*> stack;
    for (int r = 0; r < n_roots; ++r) {
        Node* root = node(roots[r]);
        if (root->buf || root->mark == ep) continue;
        root->mark = ep; stack.push_back(root);
        while (!stack.empty()) {
            Node* nd = stack.back(); stack.pop_back();
            graph.push_back(nd);
            for (int k = 0; k < nd->n_in; ++k) { Node* c = nd->in[k]; if (!c->buf && c->mark != ep) { c->mark = ep; stack.push_back(c); } }
        }
    }
    // recording order = ascending id, and a topological order: an operand exists before the operation that uses it
    std::sort(graph.begin(), graph.end(), [](const Node* a, const Node* b) { return a->id < b->id; });
}

int Engine::graph_scalars(const fmhip_vec* roots, int n_roots, double* out, int capacity) {
    require_init();
    std::vector<Node*> graph;
    collect_pending(roots, n_roots, graph);
    int count = 0;
    for (Node* nd : graph) if (op_info(nd->opcode).scalar) { if (out && count < capacity) out[count] = nd->scalar; ++count; }
    return count;
}

// The copies of a pending graph as ordinary nodes: copy j of the operations `graph` (recording order, marked ep_graph with tmp_id = position;
// substituted operands marked ep_leaf with tmp_id = i).  root_node(j, i) != nullptr: the node that is to carry operation i of copy j
// (a root that exists already: expand_replicas); otherwise a fresh node without a handle.  ids: id_of(j, i).
template <class RootNode, class IdOf, class ScalarOf, class LeafTo>
static void clone_nodes_impl(std::vector<Node*>& graph, uint64_t ep_graph, uint64_t ep_leaf, int n_copies, RootNode root_node, IdOf id_of, ScalarOf scalar_of, LeafTo leaf_to,
                             std::vector<Node*>& node_pool, std::vector<std::vector<Node*>>& copies, const std::function<void(Node*)>& pend_insert)
{
    copies.assign((size_t)n_copies, std::vector<Node*>(graph.size(), nullptr));
    for (int j = 0; j < n_copies; ++j) {
        std::vector<Node*>& copy = copies[(size_t)j];
        for (size_t i = 0; i < graph.size(); ++i) {
            const Node* src = graph[i];
            Node* nd = root_node(j, i);
            const bool fresh = nd == nullptr;
            if (fresh) {                                             // like new_node, but without a handle: inner values of a copy have none
                if (!node_pool.empty()) { nd = node_pool.back(); node_pool.pop_back(); *nd = Node(); } else nd = new Node();
                nd->id = id_of(j, i); nd->n = src->n;
            }
            nd->opcode = src->opcode; nd->n_in = src->n_in; nd->weight = src->weight;
            nd->scalar = scalar_of(j, i, src);
            for (int k = 0; k < src->n_in; ++k) {
                Node* c = src->in[k];
                Node* m = c->mark == ep_graph ? copy[(size_t)c->tmp_id] : (c->mark == ep_leaf ? leaf_to(j, c->tmp_id) : c);
                nd->in[k] = m; m->refs_int++;
            }
            if (fresh) pend_insert(nd);
            copy[i] = nd;
        }
    }
}

static const bool REPLICAS = knob_on("FMHIP_REPLICAS");     // =0: copies are always made of nodes (A/B measurement)

void Engine::graph_clone(const fmhip_vec* roots, int n_roots, int n_copies, const fmhip_vec* leaf_from, const fmhip_vec* leaf_to, int n_map,
                         const double* scalars, int n_scalars, fmhip_vec* out) {
    HostTimer timer(HostProfile::CLONE);
    require_init();
    if (n_copies < 0 || n_map < 0 || !out || (n_map > 0 && (!leaf_from || !leaf_to))) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad graph replication request");
    std::vector<Node*> graph;
    collect_pending(roots, n_roots, graph);
    const uint64_t ep_graph = ++epoch_;
    int count_scalars = 0;
    for (size_t i = 0; i < graph.size(); ++i) { graph[i]->mark = ep_graph; graph[i]->tmp_id = (int)i; count_scalars += op_info(graph[i]->opcode).scalar ? 1 : 0; }
    if (scalars && n_scalars != count_scalars)
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the graph has " + std::to_string(count_scalars) + " scalar operands, the caller supplied " + std::to_string(n_scalars));
    const uint64_t ep_leaf = ++epoch_;
    std::vector<Node*> from((size_t)n_map);
    for (int i = 0; i < n_map; ++i) {
        Node* l = node(leaf_from[i]);
        touch(l);
        if (l->mark == ep_graph) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "a substituted operand lies inside the graph to be replicated");
        l->mark = ep_leaf; l->tmp_id = i;
        from[(size_t)i] = l;
    }
    std::vector<Node*> root_nodes((size_t)n_roots);
    for (int r = 0; r < n_roots; ++r) { root_nodes[(size_t)r] = node(roots[r]); touch(root_nodes[(size_t)r]); }
    std::vector<Node*> to((size_t)n_map * (size_t)n_copies);
    for (int j = 0; j < n_copies; ++j)
        for (int i = 0; i < n_map; ++i) {
            Node* t = node(leaf_to[(size_t)j * n_map + i]);
            if (t->deferred) demand(t); else touch(t);
            if (t->n != from[(size_t)i]->n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "a substituted operand differs in size");
            to[(size_t)j * n_map + i] = t;
        }
    auto shared_root = [&](Node* root, int j) {                      // a root that is a vector already: the copy shares it (or its substitute)
        Node* c = root->mark == ep_leaf && n_map > 0 ? to[(size_t)j * n_map + root->tmp_id] : root;
        c->refs_ext++;
        if (c->refs_ext == 1 && !nodes_.get(c->id)) nodes_.put(c->id, c);
        return c->id;
    };
    // The copies as a DESCRIPTION (ReplicaGroup): only when every operand a copy would read exists as a vector already and no part of
    // the graph or of the operand map belongs to another live description.
    bool describe = REPLICAS && n_copies > 0 && !graph.empty();
    for (size_t i = 0; describe && i < graph.size(); ++i) describe = graph[i]->rep_id == 0 || replica_of(graph[i]) == nullptr;
    for (size_t i = 0; describe && i < from.size(); ++i) describe = from[i]->buf != nullptr && (from[i]->leaf_rep_id == 0 || replicas_.find(from[i]->leaf_rep_id) == replicas_.end());
    for (size_t i = 0; describe && i < to.size(); ++i) describe = to[i]->buf != nullptr;
    if (!describe) {
        std::vector<std::vector<Node*>> copies;
        clone_nodes_impl(graph, ep_graph, ep_leaf, n_copies,
                         [](int, size_t) -> Node* { return nullptr; }, [&](int, size_t) { return next_id_++; },
                         [&](int j, size_t, const Node* src) { return scalars && op_info(src->opcode).scalar ? 0.0 : src->scalar; },      // patched below (recording order)
                         [&](int j, int i) { return to[(size_t)j * n_map + i]; }, node_pool_, copies, [this](Node* nd) { pend_insert(nd); });
        for (int j = 0; j < n_copies; ++j) {
            if (scalars) { int k = 0; for (size_t i = 0; i < graph.size(); ++i) if (op_info(graph[i]->opcode).scalar) copies[(size_t)j][i]->scalar = scalars[(size_t)j * n_scalars + k++]; }
            for (int r = 0; r < n_roots; ++r) {
                Node* root = root_nodes[(size_t)r];
                if (root->mark != ep_graph) { out[(size_t)j * n_roots + r] = shared_root(root, j); continue; }
                Node* c = copies[(size_t)j][(size_t)root->tmp_id];
                c->refs_ext++;
                if (c->refs_ext == 1 && !nodes_.get(c->id)) nodes_.put(c->id, c);
                out[(size_t)j * n_roots + r] = c->id;
            }
            // copies of values nobody holds and nothing uses cannot exist: every graph node is below a root
        }
        return;
    }
    ReplicaGroup* g = new ReplicaGroup();
    g->id = next_replica_id_++;
    g->n_copies = n_copies; g->n_roots = n_roots; g->n_scalars = scalars ? n_scalars : 0;
    g->graph_size = (int)graph.size();
    g->id_base = next_id_; next_id_ += (int64_t)graph.size() * n_copies;
    g->scalar_slot.assign(graph.size(), -1);
    int slot = 0;
    for (size_t i = 0; i < graph.size(); ++i) {
        Node* nd = graph[i];
        nd->rep_id = g->id; nd->rep_index = (int32_t)i; nd->rep_root = -1; nd->rep_copy = 0;
        if (op_info(nd->opcode).scalar) g->scalar_slot[i] = slot++;
    }
    if (scalars) g->scalars.assign(scalars, scalars + (size_t)n_copies * n_scalars);
    g->leaf_from = from; g->leaf_to = to;
    for (size_t i = 0; i < from.size(); ++i) { from[i]->refs_int++; from[i]->leaf_rep_id = g->id; from[i]->leaf_rep_index = (int32_t)i; }
    for (Node* t : to) t->refs_int++;
    g->roots.assign((size_t)n_roots, nullptr);
    g->root_done.assign((size_t)n_roots, 1);
    g->copy_roots.assign((size_t)n_copies * n_roots, nullptr);
    for (int r = 0; r < n_roots; ++r) {
        Node* root = root_nodes[(size_t)r];
        if (root->mark != ep_graph) { for (int j = 0; j < n_copies; ++j) out[(size_t)j * n_roots + r] = shared_root(root, j); continue; }
        if (root->rep_root >= 0) {                                   // listed twice: the same copies again
            for (int j = 0; j < n_copies; ++j) { Node* c = g->copy_roots[(size_t)j * n_roots + root->rep_root]; c->refs_ext++; out[(size_t)j * n_roots + r] = c->id; }
            continue;
        }
        root->rep_root = r;
        root->refs_ext++;                                            // the group's hold on the original: the graph stays whole until it has run with its copies (or been expanded)
        g->roots[(size_t)r] = root; g->root_done[(size_t)r] = 0; g->remaining++;
        for (int j = 0; j < n_copies; ++j) {
            Node* c;
            if (!node_pool_.empty()) { c = node_pool_.back(); node_pool_.pop_back(); *c = Node(); } else c = new Node();
            c->id = g->id_base + (int64_t)j * g->graph_size + root->rep_index;
            c->n = root->n; c->refs_ext = 1; c->refs_int = 1;        // refs_int: the group's hold
            c->rep_id = g->id; c->rep_copy = (uint32_t)j + 1u; c->rep_root = r; c->rep_index = root->rep_index;
            nodes_.put(c->id, c);
            pend_insert(c);
            g->copy_roots[(size_t)j * n_roots + r] = c;
            out[(size_t)j * n_roots + r] = c->id;
        }
    }
    replicas_[g->id] = g;
    if (g->remaining == 0) destroy_replica_group(g);                 // (cannot happen: a non-empty graph lies below a pending root)
}

// Drops a group's holds on its operands and forgets it (its roots have all been executed, or expanded).
void Engine::destroy_replica_group(ReplicaGroup* g) {
    replicas_.erase(g->id);
    for (Node* l : g->leaf_from) { if (l->leaf_rep_id == g->id) { l->leaf_rep_id = 0; l->leaf_rep_index = -1; } node_unref_int(l); }
    for (Node* t : g->leaf_to) node_unref_int(t);
    delete g;
}

// The roots `done` (indices) have been executed together with all their copies: the copies' root nodes have their buffers.
void Engine::replica_roots_done(ReplicaGroup* g, const std::vector<int>& done) {
    for (int r : done) {
        if (g->root_done[(size_t)r]) continue;
        g->root_done[(size_t)r] = 1; g->remaining--;
        for (int j = 0; j < g->n_copies; ++j) {
            Node* c = g->copy_roots[(size_t)j * g->n_roots + r];
            c->rep_id = 0; c->rep_copy = 0; c->rep_root = -1; c->rep_index = -1;
            node_unref_int(c);
        }
        Node* root = g->roots[(size_t)r];
        root->rep_id = 0; root->rep_root = -1; root->rep_index = -1;
        if (--root->refs_ext == 0) { nodes_.erase(root->id); node_maybe_free(root); }
    }
    if (g->remaining == 0) destroy_replica_group(g);
}

// A launch sequence that was to execute these roots with their copies has FAILED midway (a device allocation, a HIP error): some
// parts or segments have committed buffers, the rest has not run.  A root whose ORIGINAL has its buffer is closed here like an executed
// one — its holds go, so the group can end and nothing leaks — and every copy of it that did NOT get its buffer is marked as lost:
// reading it is an error from now on, never a silently wrong value (a later expansion of the description skips a materialised original
// and would wire the copies' dependants to the original's vector).  Roots that have not run at all stay described, as before.
void Engine::replicas_after_failure(const std::vector<std::pair<ReplicaGroup*, std::vector<int>>>& done) {
    for (const auto& kv : done) {
        ReplicaGroup* g = kv.first;
        bool alive = false;
        for (const auto& r : replicas_) alive |= r.second == g;
        if (!alive) continue;
        // (a root whose component has run IN PART — a segment committed, a later one failed — is closed too: what is left of the original
        // reads a value the ORIGINAL's launches stored, an operation of the description with a buffer; its copies would read it as well)
        auto ran_in_part = [&](Node* root) {
            const uint64_t ep = ++epoch_;
            for (std::vector<Node*> stack{ root }; !stack.empty();) {
                Node* nd = stack.back(); stack.pop_back();
                for (int k = 0; k < nd->n_in; ++k) {
                    Node* c = nd->in[k];
                    if (c->buf && c->rep_id == g->id && !c->rep_copy) return true;
                    if (!c->buf && c->mark != ep) { c->mark = ep; stack.push_back(c); }
                }
            }
            return false;
        };
        std::vector<int> closed;
        for (int r : kv.second) {
            if (r < 0 || r >= g->n_roots || g->root_done[(size_t)r] || !g->roots[(size_t)r] || !(g->roots[(size_t)r]->buf || ran_in_part(g->roots[(size_t)r]))) continue;
            for (int j = 0; j < g->n_copies; ++j) { Node* c = g->copy_roots[(size_t)j * g->n_roots + (size_t)r]; if (c && !c->buf) c->discarded = true; }
            closed.push_back(r);
        }
        if (!closed.empty()) replica_roots_done(g, closed);
    }
}

// Fallback: the description becomes ordinary pending nodes (what graph_clone made before descriptions existed), for the roots that
// have not been executed yet.  The copies' root nodes — the handles are out — receive the root operations; every other operation of
// a copy becomes a fresh node with the id reserved for it.
void Engine::expand_replicas(ReplicaGroup* g) {
    std::vector<Node*> graph;
    {
        const uint64_t ep = ++epoch_;
        std::vector<Node*> stack;
        for (int r = 0; r < g->n_roots; ++r) {
            Node* root = g->roots[(size_t)r];
            if (!root || g->root_done[(size_t)r] || root->buf || root->mark == ep) continue;
            root->mark = ep; stack.push_back(root);
            while (!stack.empty()) {
                Node* nd = stack.back(); stack.pop_back();
                graph.push_back(nd);
                for (int k = 0; k < nd->n_in; ++k) { Node* c = nd->in[k]; if (!c->buf && c->mark != ep) { c->mark = ep; stack.push_back(c); } }
            }
        }
        std::sort(graph.begin(), graph.end(), [](const Node* a, const Node* b) { return a->id < b->id; });
    }
    const uint64_t ep_graph = ++epoch_;
    for (size_t i = 0; i < graph.size(); ++i) { graph[i]->mark = ep_graph; graph[i]->tmp_id = (int)i; }
    const uint64_t ep_leaf = ++epoch_;
    const int n_map = (int)g->leaf_from.size();
    for (int i = 0; i < n_map; ++i) { g->leaf_from[(size_t)i]->mark = ep_leaf; g->leaf_from[(size_t)i]->tmp_id = i; }
    std::vector<std::vector<Node*>> copies;
    clone_nodes_impl(graph, ep_graph, ep_leaf, g->n_copies,
                     [&](int j, size_t i) -> Node* { const Node* src = graph[i]; return src->rep_root >= 0 ? g->copy_roots[(size_t)j * g->n_roots + src->rep_root] : nullptr; },
                     [&](int j, size_t i) { return g->id_base + (int64_t)j * g->graph_size + graph[i]->rep_index; },
                     [&](int j, size_t i, const Node* src) { return g->scalar_of(j, src->rep_index, src->scalar); },
                     [&](int j, int i) { return g->leaf_to[(size_t)j * n_map + i]; }, node_pool_, copies, [this](Node* nd) { pend_insert(nd); });
    for (Node* nd : graph) { nd->rep_id = 0; nd->rep_index = -1; }   // (rep_root is cleared with the roots below)
    std::vector<int> all;
    for (int r = 0; r < g->n_roots; ++r) if (g->roots[(size_t)r] && !g->root_done[(size_t)r]) all.push_back(r);
    replica_roots_done(g, all);                                       // drops the holds; the copies' roots are ordinary pending expressions now
}

// Every live description the pending graph below `targets` touches is expanded: for the paths that execute a single expression
// (read, reduce, device_ptr, a chain passing the size threshold) instead of flushing everything.
void Engine::expand_replicas_below(const std::vector<Node*>& targets) {
    if (replicas_.empty()) return;
    for (bool again = true; again;) {
        again = false;
        const uint64_t ep = ++epoch_;
        std::vector<Node*> stack;
        for (Node* t : targets) { if (!t->buf && t->mark != ep) { t->mark = ep; stack.push_back(t); } }
        while (!stack.empty() && !again) {
            Node* nd = stack.back(); stack.pop_back();
            if (nd->rep_id) { if (ReplicaGroup* g = replica_of(nd)) { expand_replicas(g); again = true; break; } }
            for (int k = 0; k < nd->n_in; ++k) { Node* c = nd->in[k]; if (!c->buf && c->mark != ep) { c->mark = ep; stack.push_back(c); } }
        }
    }
}

// ---------------------------------------------------------------- escape policy (runtime.hpp: policy_state_)

static const bool ESCAPE_POLICY = knob_on("FMHIP_ESCAPE_POLICY");     // =0: whatever has a handle is stored (rounds 1–4; A/B measurement)

void Engine::policy_reset() { policy_state_.clear(); ++policy_gen_; }       // (shapes bind again, lazily: their generation no longer matches)

void Engine::policy_bind(ShapePolicy& p, size_t size) {
    if (p.gen != policy_gen_ || p.size != size) {
        if (policy_state_.size() + size > (size_t(1) << 28)) policy_reset();                // shapes that never repeat: start again
        p.base = (uint32_t)policy_state_.size(); p.size = (uint32_t)size; p.gen = policy_gen_;
        policy_state_.resize(policy_state_.size() + size, (uint8_t)POLICY_NEW);
        p.decided.assign(size, 0); p.flush = flush_seq_;
    } else if (p.flush != flush_seq_) { std::fill(p.decided.begin(), p.decided.end(), (uint8_t)0); p.flush = flush_seq_; }
}

// Is the value at `pos`, whose only claim to storage is a live handle, stored by this flush?  Decided once per position and flush: the
// members of a launch group must agree on their shape.  optimistic: the component comes from a caller that does not free its temporaries
// (most internally consumed values carry handles) — a position never seen is then assumed dead.
bool Engine::policy_store(ShapePolicy& p, size_t pos, bool optimistic) {
    uint8_t& d = p.decided[pos];
    if (d) return d == 1;
    uint8_t& st = policy_state_[p.base + pos];
    bool store = false;
    switch (st) {
    case POLICY_NEW:       if (optimistic) st = POLICY_DEFER; else { st = POLICY_OBSERVING; store = true; } break;
    case POLICY_OBSERVING: st = POLICY_DEFER; break;                // stored last time, and nobody came for it (touch() would have made it POLICY_STORE)
    case POLICY_STORE:     store = true; break;
    default:               break;
    }
    d = store ? 1 : 2;
    return store;
}

void Engine::defer_node(Node* nd, const ShapePolicy* p, size_t pos) {
    if (!nd->deferred) {
        pend_erase(nd);
        nd->deferred = true;
        nd->pend_prev = deferred_head_.pend_prev; nd->pend_next = &deferred_head_; deferred_head_.pend_prev->pend_next = nd; deferred_head_.pend_prev = nd;
        ++n_deferred_; ++n_deferred_total_;
    }
    if (p) watch_node(nd, *p, pos);
}

void Engine::demand(Node* nd) {
    touch(nd);
    if (!nd->buf) materialize({ nd });
}

void Engine::materialize_deferred() {
    std::vector<int64_t> ids;
    for (Node* nd = deferred_head_.pend_next; nd != &deferred_head_; nd = nd->pend_next) if (nd->refs_ext > 0) ids.push_back(nd->id);
    for (int64_t id : ids) {                        // (storing one dismantles its recipe: others may go away with it)
        Node* nd = nodes_.get(id);
        if (nd && nd->id == id && !nd->buf && nd->deferred && !nd->discarded) materialize({ nd });
    }
}

static void set_moments(Node* r, const fmhip_moments& m) { r->moments[0] = m.sum; r->moments[1] = m.sumsq; r->moments[2] = m.min; r->moments[3] = m.max; r->has_moments = true; }
static fmhip_moments moments_of(const Node* r) { return { r->moments[0], r->moments[1], r->moments[2], r->moments[3] }; }

struct Engine::Dag {
    std::vector<Node*> roots;       // the values asked for
    std::vector<Node*> order;       // pending nodes, operands before users
    std::vector<Node*> leaves;      // distinct materialised inputs
    std::vector<Node*> outs;        // roots first, then escaping intermediates
    std::vector<SsaOp> ops;
    std::vector<int> out_ids;
    std::vector<float> scalars;
    std::string sig;
    // replica descriptions (ReplicaGroup): the stamp all pending nodes of this DAG share (0: none), whether they all share one, whether any has one
    uint32_t rep_id = 0;
    bool rep_uniform = true, rep_any = false;
};

// The walk build_dag and build_big share: the pending nodes below `roots` in post-order (operands before users) into d.order, every
// node's scratch fields reset (tmp_id = -1; tmp_uses = its consumers inside the walk), the replica stamps of the pending nodes summed
// up in d.rep_id / rep_uniform / rep_any.  on_leaf(c): a materialised operand met for the first time.  Gives up (false) as soon as the
// order is longer than max_ops: too large for whoever asked, no point in walking the rest.
template <class D, class Leaf> bool Engine::walk_pending(const std::vector<Node*>& roots, D& d, size_t max_ops, Leaf&& on_leaf) {
    const uint64_t ep = ++epoch_;                   // nodes with mark == ep have been visited by THIS walk
    std::vector<std::pair<Node*, int>> stack;
    auto visit = [&](Node* nd) { nd->mark = ep; nd->tmp_id = -1; nd->tmp_uses = 0; };
    bool first_pending = true;
    auto note_rep = [&](const Node* nd) {
        if (first_pending) { d.rep_id = nd->rep_id; first_pending = false; } else if (nd->rep_id != d.rep_id) d.rep_uniform = false;
        d.rep_any |= nd->rep_id != 0;
    };
    for (Node* root : roots) {
        if (root->mark == ep) continue;             // a root that is also an operand of an earlier root
        visit(root); note_rep(root);
        stack.push_back({ root, 0 });
        while (!stack.empty()) {                    // iterative post-order
            auto& top = stack.back();
            Node* nd = top.first;
            if (top.second < nd->n_in) {
                Node* c = nd->in[top.second++];
                if (c->buf) { if (c->mark != ep) { visit(c); on_leaf(c); } }
                else { if (c->mark != ep) { visit(c); note_rep(c); stack.push_back({ c, 0 }); } c->tmp_uses++; }
            } else { d.order.push_back(nd); stack.pop_back(); if (d.order.size() > max_ops) return false; }
        }
    }
    return true;
}

// The emitter build_dag and segment_dag share: dag.order — operands before users, what they read from outside in dag.leaves — becomes SSA
// operations (ids: the leaves 0 … n_in-1, then the operations; left in the nodes' tmp_id), the scalars of the scalar-carrying ones, and
// the head of the structural signature, a short byte string (math mode, number of inputs, opcode + operand ids per op; scalars and
// vectors are NOT part of it; the caller appends the outputs).
void Engine::emit_ssa(Dag& dag) {
    const int n_in = (int)dag.leaves.size();
    for (int k = 0; k < n_in; ++k) dag.leaves[(size_t)k]->tmp_id = k;
    dag.sig.clear();
    dag.sig.reserve(dag.order.size() * 4 + 16);
    dag.sig.push_back((char)('0' + math_mode)); dag.sig.push_back((char)n_in);
    for (size_t i = 0; i < dag.order.size(); ++i) {
        Node* nd = dag.order[i];
        nd->tmp_id = n_in + (int)i;
        SsaOp op{ nd->opcode, -1, -1, -1, nd->scalar };
        int* slots[3] = { &op.a, &op.b, &op.c };
        for (int k = 0; k < nd->n_in; ++k) *slots[k] = nd->in[k]->tmp_id;
        dag.ops.push_back(op);
        if (op_info(nd->opcode).scalar) dag.scalars.push_back((float)nd->scalar);
        dag.sig.push_back((char)nd->opcode); dag.sig.push_back((char)(op.a + 1)); dag.sig.push_back((char)(op.b + 1)); dag.sig.push_back((char)(op.c + 1));
    }
    if (dag.scalars.empty()) dag.scalars.push_back(0.0f);
}

// Linearise the pending expressions below `roots` into ONE program (roots may share intermediates: they become
// several outputs of the same launch).  Returns false when it cannot run as one launch.
bool Engine::build_dag(const std::vector<Node*>& roots, Dag& dag) {
    HostTimer timer(HostProfile::BUILD_DAG);
    dag.roots = roots;
    if (!walk_pending(roots, dag, (size_t)FM_MAX_OPS, [&](Node* c) { dag.leaves.push_back(c); })) return false;
    if ((int)dag.leaves.size() > FM_MAX_IN) return false;
    emit_ssa(dag);
    // outputs: every root, plus every intermediate somebody else still needs (tmp_uses = consumers inside this DAG)
    for (Node* r : roots) if (r->tmp_uses >= 0) { dag.outs.push_back(r); dag.out_ids.push_back(r->tmp_id); r->tmp_uses = -1 - r->tmp_uses; }
    // … an intermediate with a consumer outside this DAG is a fact; one whose only claim is a live handle is the escape policy's decision
    // (1: stored, 2: a candidate, 3: not stored — deferred —, 4: a candidate the policy stores)
    const size_t n_ops = dag.order.size();
    std::vector<char> flag(n_ops, 0);
    size_t n_cand = 0, interior = 0;
    for (size_t i = 0; i < n_ops; ++i) {
        Node* nd = dag.order[i];
        if (nd->tmp_uses < 0) continue;             // already an output (root)
        ++interior;
        if (nd->refs_int > nd->tmp_uses) flag[i] = 1;
        else if (nd->refs_ext > 0) {
            if (nd->rep_id || !ESCAPE_POLICY) flag[i] = 1;
            else if (nd->deferred) flag[i] = 3;
            else { flag[i] = 2; ++n_cand; }
        }
    }
    ShapePolicy* policy = nullptr;
    if (n_cand) {
        if (dag_policies_.size() > 65536) { dag_policies_.clear(); }      // (shapes that never repeat)
        policy = &dag_policies_[dag.sig];                                  // the structural signature: nothing in it says who holds a handle
        policy_bind(*policy, n_ops);
        const bool optimistic = n_cand * 2 > interior;
        for (size_t i = 0; i < n_ops; ++i) if (flag[i] == 2) flag[i] = policy_store(*policy, i, optimistic) ? 4 : 3;
    }
    for (size_t i = 0; i < n_ops; ++i) if (flag[i] == 1 || flag[i] == 4) { dag.outs.push_back(dag.order[i]); dag.out_ids.push_back(dag.order[i]->tmp_id); }
    if ((int)dag.outs.size() > FM_MAX_OUT) return false;
    for (size_t i = 0; i < n_ops; ++i) {
        Node* nd = dag.order[i];
        if (flag[i] == 4) watch_node(nd, *policy, i);
        else if (flag[i] == 3) defer_node(nd, nd->deferred ? nullptr : policy, i);
        else if (flag[i] == 0 && nd->tmp_uses >= 0) pend_erase(nd);      // lives on as somebody's operand only: no flush starts from it
    }
    dag.sig.push_back((char)0xff);
    for (int v : dag.out_ids) dag.sig.push_back((char)(v + 1));
    return true;
}

// Execute structurally identical, mutually independent DAGs as ONE launch (one batch row per DAG).
// proto: the member that carries the structure (signature, operations); nullptr = dags[0].  Members that are copies existing as a
// description (flush_all: replica_dag) carry vectors, outputs and scalars only.
bool Engine::run_dags_plain(std::vector<Dag>& dags, const Dag* proto) {
    struct Off { bool& w; bool was; ~Off() { w = was; } } off{ want_root_moments_, want_root_moments_ };
    want_root_moments_ = false;
    return run_dags(dags, nullptr, nullptr, nullptr, proto);
}

bool Engine::run_dags(std::vector<Dag>& dags, const double* reduce_shift, fmhip_moments* host_moments, void* dev_moments, const Dag* proto) {
    HostTimer timer(HostProfile::RUN_DAGS);
    const Dag& d0 = proto ? *proto : dags[0];
    const int64_t n = dags[0].outs[0]->n;
    Program* prog = nullptr;
    if (reduce_shift && dags.size() != 1) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "a fused expectation belongs to one expression");
    // a flush that collects the moments of all pending roots (Engine::reduce): expressions of one value each, all rows of this launch
    static const double no_shift = 0.0;
    RootMoments along;                                              // (a host array or, from a flush that does not wait, slots of the pinned arena)
    bool moments_only = false;
    if (batch_trace_on()) std::fprintf(stderr, "[fmhip batch] launchable group of %zu, %zu ops, %zu outs, proto %d\n", dags.size(), d0.ops.size(), d0.out_ids.size(), proto ? 1 : 0);
    if (want_root_moments_ && !reduce_shift && !host_moments && !dev_moments && d0.out_ids.size() == 1) {
        bool roots_only = true;
        for (const Dag& d : dags) roots_only &= d.outs.size() == 1 && d.outs[0]->refs_ext > 0 && !d.outs[0]->moments_blocked;
        if (roots_only && (dags.size() >= 4 || n * (int64_t)d0.leaves.size() <= (int64_t(1) << 21) || unit_launch(n, (int64_t)dags.size()))) {
            if (along.open(*this, dags.size())) { reduce_shift = &no_shift; host_moments = along.host(); dev_moments = along.dev(); }      // (no slots: without the moments)
            // … and where the caller has given the values up (fmhip_vec_give_up_values: every member's root, nobody else holds it) the
            // launch takes the moments and stores NOTHING: a program without outputs
            // (the root of a copy that exists as a description carries one internal reference, its group's hold, until the launch is done)
            if (reduce_shift) {
                moments_only = true;
                for (const Dag& d : dags) { const Node* r = d.outs[0]; moments_only &= r->discard && r->refs_int == ((r->rep_id && r->rep_copy && replica_of(r)) ? 1 : 0); }
            }
        }
    }
    const std::string key = reduce_shift ? d0.sig + (moments_only ? "\xfeM" : "\xfeR") : d0.sig;       // the program that also reduces its root is a different program
    auto it = program_cache_.find(key);
    if (it != program_cache_.end()) prog = it->second;
    else {
        try { prog = compile(d0.ops, (int)d0.leaves.size(), moments_only ? std::vector<int>{} : d0.out_ids, reduce_shift ? std::vector<int>{ d0.out_ids[0] } : std::vector<int>{}, nullptr, false); }
        catch (const Error& e) {
            if (e.code != FMHIP_ERR_PROGRAM_LIMIT) throw;
            if (!along.is_open()) return false;
            return run_dags_plain(dags, proto);                     // without the moments, then
        }
        program_cache_[key] = prog;
    }
    std::vector<Stored> stored;
    std::vector<RowSpec> rows(dags.size());
    try {
        for (size_t i = 0; i < dags.size(); ++i) {
            for (Node* l : dags[i].leaves) rows[i].in.push_back(l->buf->ptr);
            for (size_t k = 0; k < dags[i].outs.size() && !moments_only; ++k) {
                Buffer* b = new_buffer(n);
                stored.push_back({ nullptr, 0, dags[i].outs[k], b });
                rows[i].out.push_back(b->ptr);
            }
            rows[i].scalars = dags[i].scalars.data();
            rows[i].shifts = reduce_shift;
        }
        launch(prog, n, rows, host_moments, dev_moments);
    } catch (...) {
        for (Stored& o : stored) buffer_unref(o.buf);
        throw;
    }
    if (along.is_open()) for (size_t i = 0; i < dags.size(); ++i) along.deliver(dags[i].outs[0], i);
    if (moments_only) {         // nothing was stored: the roots keep their moments, give their expressions up and are no roots of later flushes
        for (size_t i = 0; i < dags.size(); ++i) give_up_value(dags[i].outs[0]);
        return true;
    }
    commit_stored(stored);
    return true;
}

// ---------------------------------------------------------------- components larger than one launch: what they are made of, and
// build_big, which makes them (how they are planned, cut and run: plans_engine.hpp)

// What a copy that exists as a description (ReplicaGroup) needs to know about the ORIGINAL's component, per position of its order —
// taken from the nodes before anything runs (a segment's nodes are dismantled as soon as it has been committed).
struct Engine::ReplicaView {
    ReplicaGroup* g = nullptr;
    std::vector<int32_t> rep_index, rep_root;   // recording index (→ scalar slot) and root number (-1: an inner value) of the operation
    std::vector<double> scalar;                  // the original's scalar operand (copies without a scalar list use it)
};

struct Engine::BigDag {
    std::vector<Node*> roots;
    std::vector<Node*> order;       // all pending nodes of the component, operands before users
    std::vector<Node*> leaves;      // distinct materialised inputs, in discovery order (structural: equal for equal shapes)
    std::vector<char> escapes;      // per node of the order: needed outside the component (a handle, or a consumer elsewhere)
    std::string sig;                // shape: per op {opcode, operand ids (16 bit), escapes?}
    uint64_t hash = 0;              // of sig
    int64_t n = 0;                  // elements per vector
    uint32_t rep_id = 0;            // replica descriptions: as in Dag
    bool rep_uniform = true, rep_any = false;
    bool discard_root = false;      // its single root is wanted for its moments only (Node::discard; part of the signature)
    // A member WITHOUT nodes — a copy of another member's component that exists as a description: `leaves` holds the copy's operands
    // (same numbering as the original's), values produced by one launch for a later one live in `temp` (by position of the order),
    // root values also go to the copy's root nodes.
    std::shared_ptr<const ReplicaView> view;
    int copy = -1;
    std::vector<Buffer*> temp;
    bool described() const { return copy >= 0; }
    Buffer* value(size_t pos) const { return described() ? temp[pos] : order[pos]->buf; }        // nullptr: not computed (yet)
    float scalar_at(size_t pos) const {
        return (float)(described() ? view->g->scalar_of(copy, view->rep_index[pos], view->scalar[pos]) : order[pos]->scalar);
    }
};

// The STRUCTURAL signature of a list of nodes: per node its opcode and its operands (positions in the list; leaves by order of
// discovery) as one 8-byte word whose top byte — the flag: is the value stored? — stays zero; and its hash, as it is written (until
// round 4 the flag was part of it, so that a shape's identity depended on who held handles when the flush came).
static uint64_t sign_structure(const std::vector<Node*>& order, int math_mode, std::string& sig) {
    const size_t count = order.size();
    sig.resize(1 + count * 8);
    sig[0] = (char)('0' + math_mode);
    char* p = &sig[1];
    uint64_t h = 0x9e3779b97f4a7c15ull ^ (uint64_t)math_mode;
    for (size_t i = 0; i < count; ++i, p += 8) {
        const Node* nd = order[i];
        uint64_t w = (uint64_t)(uint8_t)nd->opcode;
        for (int k = 0; k < 3; ++k) w |= (uint64_t)(uint16_t)(k < nd->n_in ? nd->in[k]->tmp_id + 32768 : 0) << (8 + 16 * k);
        std::memcpy(p, &w, 8);
        h = (h ^ w) * 0xff51afd7ed558ccdull; h ^= h >> 32;
    }
    return h;
}

// the shape's full signature and hash: the structure with the flags in the top byte of every word
static void sign_flags(const std::string& structural, uint64_t structural_hash, const std::vector<char>& fl, std::string& sig, uint64_t& hash) {
    sig = structural;
    uint64_t h = structural_hash;
    for (size_t i = 0; i < fl.size(); ++i) { sig[1 + i * 8 + 7] = fl[i]; h = (h ^ ((uint64_t)(uint8_t)fl[i] + (i << 8))) * 0xff51afd7ed558ccdull; h ^= h >> 29; }
    hash = h;
}

// Schedule: the DFS post-order of the walk is A topological order, but not a good one to cut into launches — it lists a whole
// dependency chain (e.g. the running factor sum over all LIBOR components of an Euler step) before the values that merely
// consume one link of it, so every link would have to be materialised for a later segment.  List scheduling, consumers
// first: emit a ready node, then prefer the nodes it has just made ready (LIFO; ties by creation order).  A value is
// consumed as soon as possible after it is produced: short live ranges, few values crossing a cut — two Euler steps
// recorded back to back come out component by component, both steps of a component adjacent, and the intermediate state
// never touches HBM.  Every op computes the same thing in any topological order: results are unchanged bit for bit.
// PURE: reads the nodes of `order` (tmp_id = position in it), changes nothing; returns scheduled position → position in the walk.
static std::vector<uint32_t> list_schedule(const std::vector<Node*>& order) {
    const size_t m = order.size();
    std::vector<uint32_t> perm;
    perm.reserve(m);
    std::vector<int> indeg(m, 0), head(m + 1, 0);
    for (size_t i = 0; i < m; ++i)
        for (int k = 0; k < order[i]->n_in; ++k) { const Node* c = order[i]->in[k]; if (!c->buf) { indeg[i]++; head[(size_t)c->tmp_id + 1]++; } }
    for (size_t i = 0; i < m; ++i) head[i + 1] += head[i];
    std::vector<int> consumers((size_t)head[m]), fill(head.begin(), head.end() - 1);
    for (size_t i = 0; i < m; ++i)
        for (int k = 0; k < order[i]->n_in; ++k) { const Node* c = order[i]->in[k]; if (!c->buf) consumers[(size_t)fill[(size_t)c->tmp_id]++] = (int)i; }
    auto by_id_desc = [&](int a, int b) { return order[(size_t)a]->id > order[(size_t)b]->id; };
    std::vector<int> stack_ready;
    for (size_t i = 0; i < m; ++i) if (indeg[i] == 0) stack_ready.push_back((int)i);
    std::sort(stack_ready.begin(), stack_ready.end(), by_id_desc);             // oldest node on top
    std::vector<int> fresh;
    while (!stack_ready.empty()) {
        const int i = stack_ready.back(); stack_ready.pop_back();
        perm.push_back((uint32_t)i);
        fresh.clear();
        for (int q = head[(size_t)i]; q < head[(size_t)i + 1]; ++q) if (--indeg[(size_t)consumers[(size_t)q]] == 0) fresh.push_back(consumers[(size_t)q]);
        std::sort(fresh.begin(), fresh.end(), by_id_desc);
        stack_ready.insert(stack_ready.end(), fresh.begin(), fresh.end());
    }
    if (perm.size() != m) { perm.resize(m); for (size_t i = 0; i < m; ++i) perm[i] = (uint32_t)i; }      // (never: the pending graph is acyclic)
    return perm;
}

// build_big, step 2 — the order of the walk becomes the scheduled order (every node's tmp_id = its position in it).  A shape seen before
// (same walk, same operands) is scheduled the way it was then: the schedule is a function of the structure up to ties, and any
// topological order computes the same values — a caller that asks for one expectation after the other (144 products per objective
// evaluation, each a graph of 50–250 nodes) pays for the walk and ONE signature, not for the scheduling pass and a second one (≈ 6 →
// 3 µs per product, all of it time the device waits).  Returns the shape's memo — it also carries what the engine has learnt about the
// shape's handles (escape policy) and the variants it has used —, nullptr for a component too large to remember.
Engine::ScheduleMemo* Engine::schedule_big(BigDag& big) {
    static const size_t MEMO_MAX_NODES = 16384;               // (a memo holds ≈ 30 bytes per node)
    const size_t m = big.order.size();
    for (size_t i = 0; i < m; ++i) big.order[i]->tmp_id = (int)i;
    ScheduleMemo* memo = nullptr;
    if (m <= MEMO_MAX_NODES) {
        const uint64_t walk_hash = sign_structure(big.order, math_mode, walk_sig_);
        auto known = schedule_cache_.find(walk_hash);
        if (known != schedule_cache_.end() && known->second.walk_sig == walk_sig_) memo = &known->second;
        else {
            if (schedule_cache_.size() >= 4096 || schedule_cache_bytes_ > (size_t(128) << 20)) { schedule_cache_.clear(); schedule_cache_bytes_ = 0; policy_reset(); }     // (shapes that never repeat: start again)
            memo = &schedule_cache_[walk_hash];
            schedule_cache_bytes_ -= std::min(schedule_cache_bytes_, memo->walk_sig.size() * 3 + memo->perm.size() * 6);       // (the same walk hash again: replaced)
            *memo = ScheduleMemo();
            memo->walk_sig = walk_sig_;
        }
    }
    const bool known = memo && !memo->perm.empty();
    std::vector<uint32_t> fresh;
    if (!known) fresh = list_schedule(big.order);
    const std::vector<uint32_t>& perm = known ? memo->perm : fresh;
    std::vector<Node*> scheduled(m);
    for (size_t i = 0; i < m; ++i) { scheduled[i] = big.order[perm[i]]; scheduled[i]->tmp_id = (int)i; }
    big.order.swap(scheduled);
    if (memo && !known) {
        memo->perm.swap(fresh);
        memo->sched_hash = sign_structure(big.order, math_mode, memo->sched_sig);
        schedule_cache_bytes_ += memo->walk_sig.size() * 3 + memo->perm.size() * 6;
    }
    return memo;
}

// build_big, step 3 — which values are stored.  A consumer outside the component, or being a root of this walk, is a fact; a value whose
// only claim is a live handle is the escape policy's decision ('?' → 'x' stored and watched / '.' deferred); 'd': deferred earlier,
// stays so.  facts: the flags before the policy spoke ('x' / 'm' there are facts; '?' and 'd' the policy's to decide, '.' nobody's).
// Changes policy state only (policy_bind / policy_store), no node.
void Engine::store_flags(const BigDag& big, ScheduleMemo* memo, std::vector<char>& flags, std::vector<char>& facts) {
    const size_t m = big.order.size();
    flags.resize(m);
    size_t n_cand = 0, interior = 0;
    for (size_t i = 0; i < m; ++i) {
        const Node* nd = big.order[i];
        // (a root whose VALUE the caller has given up — moments only, Node::discard — is not an output of the component: 'm', a shape of
        // its own, its peeled kernels do not store it; launches that cannot take the moments along — segments — store it all the same)
        char f = '.';
        if (nd->discard && nd->refs_int == 0) f = 'm';
        else if (nd->refs_int > nd->tmp_uses) f = 'x';
        else if (nd->refs_ext > 0) {
            if (nd->tmp_uses == 0 || nd->rep_id || !memo || !ESCAPE_POLICY) f = 'x';
            else if (nd->deferred) f = 'd';
            else { f = '?'; ++n_cand; }
        }
        interior += nd->tmp_uses > 0 ? 1 : 0;
        flags[i] = f;
    }
    facts = flags;
    if (n_cand) {
        policy_bind(memo->policy, m);
        const bool optimistic = n_cand * 2 > interior;
        for (size_t i = 0; i < m; ++i) if (flags[i] == '?') flags[i] = policy_store(memo->policy, i, optimistic) ? 'x' : '.';
    }
    for (size_t i = 0; i < m; ++i) if (flags[i] == 'd') flags[i] = '.';
}

// The hysteresis of choose_variant: the wanted variant `at` of the shape, or — while its kernel is still being compiled — the variant
// used last whose kernel exists and which stores every value somebody outside the component needs (the facts).  A wanted variant that
// was never planned is planned here (its loop is looked for, its kernels are asked for; nothing runs).
size_t Engine::variant_with_kernel(BigDag& big, ScheduleMemo& memo, size_t at, const std::vector<char>& flags, const std::vector<char>& facts) {
    std::vector<ScheduleMemo::Variant>& vs = memo.variants;
    const size_t m = big.order.size();
    auto plan_of = [&](const ScheduleMemo::Variant& v) -> BigPlan* { auto it = plan_cache_.find(v.hash); return it != plan_cache_.end() && it->second.sig == v.sig ? &it->second : nullptr; };
    auto kernel_there = [&](const BigPlan& p) {
        if (!p.rolled.present) return true;
        const std::shared_ptr<JitSlot>& slot = p.rolled.peeled.present ? p.rolled.peeled.jit : p.rolled.jit;
        return slot && slot->state.load(std::memory_order_acquire) != JitSlot::QUEUED;
    };
    BigPlan* wanted = plan_of(vs[at]);
    if (!wanted && plan_cache_.count(vs[at].hash) == 0) {
        big.escapes.resize(m);
        for (size_t i = 0; i < m; ++i) big.escapes[i] = flags[i] == 'x' ? 1 : 0;
        BigPlan np;
        plan_loop(np, big);
        np.sig = vs[at].sig; np.discards_root = big.discard_root; np.segs_missing = true;
        wanted = &(plan_cache_[vs[at].hash] = std::move(np));
    }
    if (!wanted || kernel_there(*wanted)) return at;
    for (size_t back = memo.last_variant < vs.size() ? memo.last_variant : 0, tried = 0; tried < vs.size(); ++tried, back = (back + 1) % vs.size()) {
        if (back == at) continue;
        const ScheduleMemo::Variant& v = vs[back];
        bool legal = true;
        for (size_t i = 0; i < m && legal; ++i) legal = (facts[i] != 'x' || v.flags[i] == 'x') && ((facts[i] == 'm') == (v.flags[i] == 'm'));
        if (!legal) continue;
        const BigPlan* p = plan_of(v);
        if (p && kernel_there(*p)) return back;
    }
    return at;
}

// build_big, step 4 — the shape's signature and hash (big.sig / big.hash) for the flags decided, through the VARIANTS of this shape —
// the same structure, other values stored — the engine has used: the escape policy moves a shape through a few of them while it learns
// (stored for observation → left unstored → stored after all), and each needs its own loop kernel.  A variant whose kernel is still
// being compiled does not run as segments on the interpreter meanwhile: the launch goes through the variant used last whose kernel
// exists (variant_with_kernel; `flags` become that variant's) — a value stored without need costs a write, one left unstored against the
// policy's wish is computed from its recipe if somebody asks (and watched all the same).  The wanted variant's kernel is asked for now,
// and used once it is there.  Changes the memo (variants, last_variant, the accounting of its bytes) and the plan cache, no node.
void Engine::choose_variant(BigDag& big, ScheduleMemo* memo, std::vector<char>& flags, const std::vector<char>& facts) {
    if (!memo) { std::string structural; const uint64_t h = sign_structure(big.order, math_mode, structural); sign_flags(structural, h, flags, big.sig, big.hash); return; }
    std::vector<ScheduleMemo::Variant>& vs = memo->variants;
    size_t at = vs.size();
    for (size_t v = 0; v < vs.size(); ++v) if (vs[v].flags == flags) { at = v; break; }
    if (at == vs.size()) {
        if (vs.size() >= 6) { vs.erase(vs.begin() + 1, vs.begin() + 2); at = vs.size(); }     // (the oldest but the first — the one that stores everything it was asked to at first sight)
        vs.emplace_back();
        vs[at].flags = flags;
        sign_flags(memo->sched_sig, memo->sched_hash, flags, vs[at].sig, vs[at].hash);
        schedule_cache_bytes_ += vs[at].sig.size() + big.order.size();
    }
    size_t use = at;
    static const bool HYSTERESIS = knob_on("FMHIP_VARIANT_HYSTERESIS");
    if (HYSTERESIS && ESCAPE_POLICY && vs.size() > 1 && jit_mode == FMHIP_JIT_AUTO) use = variant_with_kernel(big, *memo, at, flags, facts);
    memo->last_variant = use;
    if (use != at) flags = vs[use].flags;
    big.sig = vs[use].sig; big.hash = vs[use].hash;
}

// build_big, step 5 — the nodes learn what has been decided (and big.escapes says it per position): a handle whose value is stored is
// watched (watch_node: a use makes its position a stored one for good), one whose value is not is deferred (defer_node); whatever lives
// on as somebody's operand only leaves the pending list (pend_erase) — no flush starts from it.
void Engine::teach_nodes(BigDag& big, ScheduleMemo* memo, const std::vector<char>& flags, const std::vector<char>& facts) {
    const size_t m = big.order.size();
    big.escapes.resize(m);
    for (size_t i = 0; i < m; ++i) {
        Node* nd = big.order[i];
        if (flags[i] == 'x') { if (facts[i] == '?') watch_node(nd, memo->policy, i); }
        else if (flags[i] == '.') {
            if (nd->refs_ext > 0 && nd->tmp_uses > 0 && nd->refs_int <= nd->tmp_uses) defer_node(nd, facts[i] == '?' ? &memo->policy : nullptr, i);
            else if (!nd->deferred) pend_erase(nd);
        }
        big.escapes[i] = flags[i] == 'x' ? 1 : 0;
    }
}

// A component that does not fit one launch, ready to be planned and run: walked (step 1: the walk of build_dag; leaves numbered -1,
// -2, … in tmp_id), scheduled (schedule_big), its stored values decided (store_flags), signed (choose_variant), its nodes told
// (teach_nodes).  Only the last step touches the pending list.  false: too large even for that.
bool Engine::build_big(const std::vector<Node*>& roots, BigDag& big) {
    HostTimer timer(HostProfile::BUILD_BIG);
    big.roots = roots;
    big.leaves.clear();
    big.n = roots[0]->n;
    big.discard_root = roots.size() == 1 && roots[0]->discard && roots[0]->refs_int == 0;
    int n_leaves = 0;
    walk_pending(roots, big, ~size_t(0), [&](Node* c) { c->tmp_id = --n_leaves; big.leaves.push_back(c); });
    if (big.order.size() > 60000) return false;
    ScheduleMemo* memo = schedule_big(big);
    std::vector<char> flags, facts;
    store_flags(big, memo, flags, facts);
    choose_variant(big, memo, flags, facts);
    teach_nodes(big, memo, flags, facts);
    return true;
}

// Commit: what a launch has stored becomes materialised vectors; their expressions (and unreferenced intermediates) go away.  All
// outputs are kept alive until every expression has been dismantled: one that nobody holds — stored for the sake of a launch shape whose
// kernel exists (build_big), a position a loop stores in every iteration for the sake of one — goes away with its last consumer.
void Engine::commit_stored(const std::vector<Stored>& outs) {
    std::vector<Node*> done;
    done.reserve(outs.size());
    for (const Stored& o : outs) {
        if (o.big && o.big->described()) { commit_described(*o.big, o.pos, o.buf); continue; }
        Node* nd = o.big ? o.big->order[o.pos] : o.node;
        commit_node(nd, o.buf);
        done.push_back(nd);
    }
    for (Node* nd : done) nd->refs_int++;
    for (Node* nd : done) drop_expression(nd);
    for (Node* nd : done) { nd->refs_int--; node_maybe_free(nd); }
}

void Engine::give_up_value(Node* r) { r->discarded = true; r->refs_int++; drop_expression(r); r->refs_int--; }

static const bool MERGE_CHAINS = knob_on("FMHIP_MERGE_CHAINS");          // =0: off (merged_chains_engine.hpp)

// A launch sequence that executes replicated roots with their copies that exist as a description: the scope guard of the flush, in the
// spirit of PassOutputs::commit.  It owns the list of what is executed (per description, the roots by index) and ends in one of three
// ways: finish() — everything ran, the roots are done; dismiss() — the group did not run as a group (its roots go on as leftovers or are
// computed one by one), the descriptions stay as they are; fail() — also what the destructor does to a guard still open, i.e. on an
// exception from anywhere in the flush: replicas_after_failure, which leaves a root whose original has NO buffer described — a no-op
// for a group that has not run at all.
struct Engine::ReplicaLaunch {
    Engine* e;
    std::vector<std::pair<ReplicaGroup*, std::vector<int>>> done;
    bool open = true;
    explicit ReplicaLaunch(Engine* engine) : e(engine) {}
    ReplicaLaunch(ReplicaLaunch&& o) noexcept : e(o.e), done(std::move(o.done)), open(o.open) { o.open = false; }      // (move only)
    void finish() { if (open) { open = false; for (auto& kv : done) e->replica_roots_done(kv.first, kv.second); } }
    void dismiss() { open = false; }
    void fail() { if (open) { open = false; e->replicas_after_failure(done); } }
    ~ReplicaLaunch() { fail(); }
};

struct Engine::SmallGroup { std::vector<Dag> members; Dag proto; const SmallMatch* match = nullptr; ReplicaLaunch launch; explicit SmallGroup(Engine* e) : launch(e) {} };
struct Engine::BigGroups { std::vector<std::vector<BigDag>> members; std::vector<ReplicaLaunch> launches; };       // per group of one shape: its members and its guard

bool Engine::try_fused(const std::vector<Node*>& roots) {
    std::vector<Dag> dags(1);
    if (!build_dag(roots, dags[0])) return false;
    return run_dags(dags);
}

void Engine::materialize(const std::vector<Node*>& targets) {
    ++flush_seq_;
    for (Node* t : targets)
        if (t->discarded && !t->buf) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the value of this vector does not exist: it was given up (fmhip_vec_give_up_values: only its moments were taken), or lost in a launch that failed");
    expand_replicas_below(targets);                 // a single expression is executed, not everything pending: descriptions of copies it touches become nodes first
    for (Node* t : targets) {
        if (t->buf) continue;
        if (try_fused({ t })) continue;
        // Too large for one launch: cut the component into consecutive segments (run_big_group)
        std::vector<BigDag> one(1);
        if (!build_big({ t }, one[0])) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "expression too large");
        run_big_group(one);
    }
}

// ---------------------------------------------------------------- the flush (flush_all, below, is a driver over these steps)

// Step 1 — the live pending vectors nobody pending depends on, by id.  Reads the pending list, changes nothing.  false: there is none.
bool Engine::pending_roots(std::vector<Node*>& roots) {
    for (Node* nd = pending_head_.pend_next; nd != &pending_head_; nd = nd->pend_next) if (nd->refs_int == 0 && nd->refs_ext > 0 && !nd->discarded) roots.push_back(nd);
    std::sort(roots.begin(), roots.end(), [](Node* a, Node* b) { return a->id < b->id; });
    return !roots.empty();
}
// … and where there is none: a live pending node, if any (an operand of dead ones)
Node* Engine::any_live_pending() {
    for (Node* nd = pending_head_.pend_next; nd != &pending_head_; nd = nd->pend_next) if (nd->refs_ext > 0 && !nd->discarded) return nd;
    return nullptr;
}

// Step 2 — the connected components of the pending graph below `roots` (union-find over root indices): per component its roots, the
// components in the order of their first root.  Uses the nodes' scratch fields (mark, tmp_id), changes nothing else.
void Engine::pending_components(const std::vector<Node*>& roots, OrderedGroups<int, Node*>& comps) {
    std::vector<int> parent(roots.size());
    for (size_t i = 0; i < roots.size(); ++i) parent[i] = (int)i;
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    const uint64_t ep = ++epoch_;
    std::vector<Node*> stack;
    for (size_t i = 0; i < roots.size(); ++i) {
        stack.push_back(roots[i]);
        roots[i]->mark = ep; roots[i]->tmp_id = (int)i;
        while (!stack.empty()) {
            Node* nd = stack.back(); stack.pop_back();
            for (int k = 0; k < nd->n_in; ++k) {
                Node* c = nd->in[k];
                if (c->buf) continue;
                if (c->mark == ep) { const int a = find((int)i), b = find(c->tmp_id); if (a != b) parent[b] = a; }
                else { c->mark = ep; c->tmp_id = (int)i; stack.push_back(c); }
            }
        }
    }
    for (size_t i = 0; i < roots.size(); ++i) comps[find((int)i)].push_back(roots[i]);
}

// A component of a replicated graph runs with its copies as further rows — if it still is exactly what was replicated: all its
// operations belong to ONE live description (rep_id, uniform) and nothing but the replicated roots escapes from it (escapes: per node,
// nullptr = every node of `nodes` escapes).  Otherwise every description the pending graph below `roots` touches becomes ordinary nodes
// (expand_replicas_below); true when that changed anything: the round starts again on the larger pending graph (an expansion may
// release nodes other components were found through).
bool Engine::expand_unless_whole(uint32_t rep_id, bool uniform, const std::vector<Node*>& nodes, const std::vector<char>* escapes, const std::vector<Node*>& roots) {
    ReplicaGroup* g = clean_replica_group(rep_id, uniform);
    for (size_t i = 0; g && i < nodes.size(); ++i) if ((!escapes || (*escapes)[i]) && (nodes[i]->rep_root < 0 || nodes[i]->rep_copy)) g = nullptr;
    if (g) return false;
    const size_t before = replicas_.size();
    expand_replicas_below(roots);
    return replicas_.size() != before;
}

// Step 3 — one Dag per component, grouped by structure and vector length (first-seen order); the roots of components that do not fit
// one launch go to `leftovers`.  build_dag takes interior nodes off the pending list and defers what the escape policy leaves unstored.
// false: a description was expanded (expand_unless_whole) — the pending graph has grown, the caller starts the round again.
bool Engine::small_groups(OrderedGroups<int, Node*>& comps, OrderedGroups<std::string, Dag>& groups, std::vector<Node*>& leftovers) {
    for (std::vector<Node*>& comp : comps.lists) {
        Dag d;
        if (!build_dag(comp, d)) { for (Node* r : comp) leftovers.push_back(r); continue; }
        if (d.rep_any && expand_unless_whole(d.rep_id, d.rep_uniform, d.outs, nullptr, comp)) return false;
        std::string key = d.sig; key.push_back('#'); key += std::to_string(d.roots[0]->n);
        groups[key].push_back(std::move(d));
    }
    return true;
}

// What a launch group needs of a component that runs with its described copies: the replicated roots it executes (a BigDag also writes
// down what its copies need to know once its nodes are gone: the ReplicaView all of them share) …
std::vector<int> Engine::replicated_roots(Dag& d, ReplicaGroup*) {
    std::vector<int> roots;
    for (Node* o : d.outs) roots.push_back(o->rep_root);
    return roots;
}
std::vector<int> Engine::replicated_roots(BigDag& b, ReplicaGroup* g) {
    auto view = std::make_shared<ReplicaView>();
    view->g = g;
    const size_t m = b.order.size();
    view->rep_index.resize(m); view->rep_root.resize(m); view->scalar.resize(m);
    std::vector<int> roots;
    for (size_t i = 0; i < m; ++i) {
        const Node* nd = b.order[i];
        view->rep_index[i] = nd->rep_index; view->rep_root[i] = nd->rep_root; view->scalar[i] = nd->scalar;
        if (nd->rep_root >= 0) roots.push_back(nd->rep_root);
    }
    b.view = std::move(view);
    return roots;
}
// … and copy `copy` as a member of its own: the vectors it reads, the root nodes that receive its results, its scalars.
Engine::Dag Engine::replica_member(const Dag& d, ReplicaGroup* g, int copy) {
    Dag r;
    r.leaves.reserve(d.leaves.size());
    for (Node* l : d.leaves) r.leaves.push_back(g->leaf_of(copy, l));
    r.outs.reserve(d.outs.size());
    for (Node* o : d.outs) r.outs.push_back(g->copy_roots[(size_t)copy * g->n_roots + (size_t)o->rep_root]);
    for (const Node* nd : d.order) if (op_info(nd->opcode).scalar) r.scalars.push_back((float)g->scalar_of(copy, nd->rep_index, nd->scalar));
    if (r.scalars.empty()) r.scalars.push_back(0.0f);
    return r;
}
Engine::BigDag Engine::replica_member(const BigDag& b, ReplicaGroup* g, int copy) {
    BigDag r;
    r.n = b.n; r.view = b.view; r.copy = copy;
    r.leaves.reserve(b.leaves.size());
    for (Node* l : b.leaves) r.leaves.push_back(g->leaf_of(copy, l));
    r.temp.assign(b.order.size(), nullptr);
    return r;
}

// The members of a launch group: every component of `originals`, each followed by its copies that exist as a description; the roots
// they execute are written into the group's guard.
template <class D> void Engine::members_with_copies(std::vector<D>& originals, std::vector<D>& members, ReplicaLaunch& launch) {
    for (D& d : originals) {
        ReplicaGroup* g = d.rep_any ? clean_replica_group(d.rep_id, d.rep_uniform) : nullptr;
        if (!g) { members.push_back(std::move(d)); continue; }
        launch.done.push_back({ g, replicated_roots(d, g) });
        const size_t at = members.size();
        members.push_back(std::move(d));
        for (int j = 0; j < g->n_copies; ++j) members.push_back(replica_member(members[at], g, j));
    }
}

// The launches of a small group, MAX_LAUNCH_ROWS members each.  A part that does not run as one launch after all gives its roots to `leftovers`
// (they run as large components) or, late (leftovers == nullptr: behind the large components), computes them one by one; the group's
// descriptions are then left alone (dismiss), otherwise its roots are done (finish).  An exception leaves the guard open.
void Engine::run_small(SmallGroup& sg, std::vector<Node*>* leftovers) {
    bool ran = true;
    for (size_t off = 0; off < sg.members.size(); off += MAX_LAUNCH_ROWS) {
        std::vector<Dag> part(std::make_move_iterator(sg.members.begin() + off), std::make_move_iterator(sg.members.begin() + std::min(sg.members.size(), off + MAX_LAUNCH_ROWS)));
        if (run_dags(part, nullptr, nullptr, nullptr, &sg.proto)) continue;
        ran = false;
        for (Dag& d : part) for (Node* r : d.roots) { if (leftovers) leftovers->push_back(r); else if (!r->buf) materialize({ r }); }
    }
    if (ran) sg.launch.finish(); else sg.launch.dismiss();
}

// Step 4 — one group of structurally identical components (`g`, consumed) with their described copies: run now, or — a group whose
// components may be chains of a merged launch (merge_families) — parked in `waiting`, behind the large components.  Commits buffers and
// dismantles the expressions that ran; an exception closes the group here (its guard is a local), the parked ones are the driver's.
void Engine::run_small_group(std::vector<Dag>& g, std::vector<SmallGroup>& waiting, std::vector<Node*>& leftovers) {
    SmallGroup sg(this);
    sg.proto = g[0];                                          // carries the structure for launches that start with another member
    sg.match = (MERGE_CHAINS && want_root_moments_ && jit_mode != FMHIP_JIT_OFF) ? match_small(sg.proto) : nullptr;
    members_with_copies(g, sg.members, sg.launch);
    if (sg.match) waiting.push_back(std::move(sg)); else run_small(sg, &leftovers);
}

// The parked groups, late: what merge_families has left of them (nothing: their roots are done).
void Engine::run_parked(std::vector<SmallGroup>& waiting) {
    for (SmallGroup& sg : waiting) { if (!sg.members.empty()) run_small(sg, nullptr); else sg.launch.finish(); }
    waiting.clear();
}

// Step 5 — the components `leftovers` belong to (they do not fit one launch) as BigDags, grouped by a 64-bit hash of (shape signature,
// vector length) — the signatures are ~10 KB strings, hashed ONCE in build_big —, first-seen order; then per group its members with
// their described copies and its guard.  build_big defers and un-pends nodes as build_dag does.  false: a description was expanded.
bool Engine::big_groups(OrderedGroups<int, Node*>& comps, const std::vector<Node*>& leftovers, BigGroups& big) {
    std::unordered_map<Node*, size_t> comp_of;                    // root -> component
    for (size_t c = 0; c < comps.lists.size(); ++c) for (Node* r : comps.lists[c]) comp_of[r] = c;
    std::unordered_set<size_t> big_comps;
    std::vector<size_t> big_order;
    for (Node* r : leftovers) { const size_t c = comp_of[r]; if (big_comps.insert(c).second) big_order.push_back(c); }
    OrderedGroups<uint64_t, BigDag> shapes;
    for (size_t c : big_order) {
        std::vector<Node*> roots;
        for (Node* r : comps.lists[c]) if (!r->buf) roots.push_back(r);
        if (roots.empty()) continue;
        BigDag b;
        if (!build_big(roots, b)) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "pending expression too large");
        if (b.rep_any && expand_unless_whole(b.rep_id, b.rep_uniform, b.order, &b.escapes, roots)) return false;
        uint64_t key = b.hash ^ ((uint64_t)roots[0]->n * 0x9E3779B97F4A7C15ull);
        std::vector<BigDag>* members = &shapes[key];
        if (!members->empty() && ((*members)[0].sig != b.sig || (*members)[0].roots[0]->n != roots[0]->n))      // hash collision (practically never): a group of its own
            members = &shapes[key * 0xff51afd7ed558ccdull + shapes.lists.size() + 1];
        members->push_back(std::move(b));
    }
    big.members.resize(shapes.lists.size());
    big.launches.reserve(shapes.lists.size());
    for (size_t k = 0; k < shapes.lists.size(); ++k) { big.launches.emplace_back(this); members_with_copies(shapes.lists[k], big.members[k], big.launches[k]); }
    return true;
}

// Step 6 — components of one loop shape that read the same vectors, one a suffix of the other's, as one launch per family size
// (merge_families: it takes chains out of the big groups and out of the parked small groups); then the parked groups, then the big
// groups (run_big_group: planned, cut into segments; components of identical shape share the cuts and the launches).
void Engine::run_big_groups(BigGroups& big, std::vector<SmallGroup>& waiting) {
    merge_families(big.members, waiting);
    run_parked(waiting);
    for (size_t k = 0; k < big.members.size(); ++k) {
        if (!big.members[k].empty()) run_big_group(big.members[k]);
        big.launches[k].finish();
    }
}

// Execute everything that is pending and still referenced.  Pending results that share intermediates form one
// connected component and run as ONE multi-output launch; components with identical structure (same ops, different
// vectors and scalars — e.g. all LIBOR components of an Euler step) are batched as rows of one launch.
void Engine::flush_all() {
    HostTimer timer(HostProfile::FLUSH);
    require_init();
    if (late_count() >= late_eager()) drain_late();
    ++flush_seq_;
    for (int round = 0; round < 1000000; ++round) {
        std::vector<Node*> roots;
        OrderedGroups<int, Node*> comps;
        {
            HostTimer t_components(HostProfile::FLUSH_COMPONENTS);
            if (!pending_roots(roots)) {                          // only operands of dead nodes are left: one live one is computed on its own, then again
                Node* live = any_live_pending();
                if (!live) return;
                materialize({ live });
                continue;
            }
            pending_components(roots, comps);
        }
        OrderedGroups<std::string, Dag> small;
        std::vector<Node*> leftovers;
        if (!small_groups(comps, small, leftovers)) continue;     // a description was expanded: again, on the larger pending graph
        std::vector<SmallGroup> waiting;                           // groups parked behind the large components (run_small_group)
        BigGroups big;
        try {
            for (std::vector<Dag>& g : small.lists) run_small_group(g, waiting, leftovers);
            if (leftovers.empty()) { run_parked(waiting); continue; }                             // nothing large in this flush: the parked groups have no family to join
            if (!big_groups(comps, leftovers, big)) { run_parked(waiting); continue; }            // expanded: again
            run_big_groups(big, waiting);
        } catch (...) {
            // every group still in flight is closed, in this order: the big groups as they were to run, then the parked ones
            for (ReplicaLaunch& l : big.launches) l.fail();
            for (SmallGroup& sg : waiting) sg.launch.fail();
            throw;
        }
    }
}

// ---------------------------------------------------------------- explicit programs

fmhip_program Engine::program_create(const fmhip_prog_op* ops, int n_ops, int n_in, const int32_t* outs, int n_out,
                                     const int32_t* reds, int n_red) {
    require_init();
    if (n_ops < 0 || n_out < 0 || n_red < 0 || (n_ops > 0 && !ops) || (n_out > 0 && !outs) || (n_red > 0 && !reds))
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad program description");
    if (n_out == 0 && n_red == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "a program needs an output or a reduction");
    std::vector<SsaOp> s(n_ops);
    for (int i = 0; i < n_ops; ++i) s[i] = { ops[i].opcode, ops[i].a, ops[i].b, ops[i].c, ops[i].scalar };
    Program* p = compile(s, n_in, std::vector<int>(outs, outs + n_out), std::vector<int>(reds, reds + n_red), nullptr, true);
    if (jit_mode != FMHIP_JIT_OFF) p->jit = jit().request(p->proto, jit_mode == FMHIP_JIT_SYNC);    // explicit = declared hot
    const int64_t id = next_id_++;
    programs_[id] = p;
    return id;
}

std::string Engine::program_source(const fmhip_prog_op* ops, int n_ops, int n_in, const int32_t* outs, int n_out, const int32_t* reds, int n_red) {
    if (n_ops < 0 || n_out < 0 || n_red < 0 || (n_ops > 0 && !ops) || (n_out > 0 && !outs) || (n_red > 0 && !reds))
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad program description");
    std::vector<SsaOp> s(n_ops);
    for (int i = 0; i < n_ops; ++i) s[i] = { ops[i].opcode, ops[i].a, ops[i].b, ops[i].c, ops[i].scalar };
    std::unique_ptr<Program> p(compile(s, n_in, std::vector<int>(outs, outs + n_out), std::vector<int>(reds, reds + n_red), nullptr, true));
    return jit_generate_source(p->proto);
}

Program* Engine::program(fmhip_program h) {
    auto it = programs_.find(h);
    if (it == programs_.end()) throw Error(FMHIP_ERR_INVALID_HANDLE, "invalid program handle " + std::to_string(h));
    return it->second;
}

void Engine::program_release(fmhip_program h) {
    require_init();
    Program* p = program(h);
    programs_.erase(h);
    if (--p->refs == 0) delete p;
}

void Engine::program_run(fmhip_program h, int batch, const fmhip_vec* inputs, fmhip_vec* outputs, bool into,
                         const double* shifts, fmhip_moments* moments, void* dev_moments) {
    require_init();
    Program* p = program(h);
    if (batch <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "batch must be positive");
    if (!inputs || (p->n_out > 0 && !outputs)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "null handle array");
    std::vector<RowSpec> rows(batch);
    std::vector<Node*> in_nodes((size_t)batch * p->n_in);
    int64_t n = -1;
    for (int b = 0; b < batch; ++b)
        for (int k = 0; k < p->n_in; ++k) {
            Node* nd = node(inputs[(size_t)b * p->n_in + k]);
            if (n < 0) n = nd->n;
            if (nd->n != n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "program inputs differ in size");
            in_nodes[(size_t)b * p->n_in + k] = nd;
        }
    for (Node* nd : in_nodes) { touch(nd); if (!nd->buf) materialize({ nd }); }
    std::vector<Buffer*> fresh;
    std::vector<Node*> out_nodes;
    try {
        for (int b = 0; b < batch; ++b) {
            for (int k = 0; k < p->n_in; ++k) rows[b].in.push_back(in_nodes[(size_t)b * p->n_in + k]->buf->ptr);
            for (int k = 0; k < p->n_out; ++k) {
                if (into) {
                    Node* o = node(outputs[(size_t)b * p->n_out + k]);
                    if (o->n != n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "program output differs in size");
                    touch(o);
                    if (!o->buf) materialize({ o });
                    if (o->refs_int > 0) { flush_all(); materialize_deferred(); }      // overwritten in place: whoever still reads the old contents (pending expressions, recipes of deferred values) is computed first
                    o->has_moments = false; o->moments_slot = nullptr;      // overwritten
                    make_private(o);
                    rows[b].out.push_back(o->buf->ptr);
                } else {
                    Buffer* bf = new_buffer(n);
                    fresh.push_back(bf);
                    rows[b].out.push_back(bf->ptr);
                }
            }
            rows[b].scalars = nullptr;
            rows[b].shifts = shifts;
        }
        launch(p, n, rows, moments, dev_moments);
    } catch (...) { for (Buffer* b : fresh) buffer_unref(b); throw; }
    if (!into)
        for (size_t i = 0; i < fresh.size(); ++i) { Node* nd = new_node(n); nd->buf = fresh[i]; outputs[i] = nd->id; }
}

// ---------------------------------------------------------------- brownian increments

// The vectors of one generation share ONE block of the pool: n_streams vectors `*stride` floats apart (every vector 256-B aligned), which
// `fill(first vector)` writes; if it throws, the block goes back to the pool.  The slab itself has no handle: its views keep it (slab_views).
template <class Fill>
Buffer* Engine::slab_generate(int64_t n_paths, int64_t n_streams, int64_t* stride, Fill fill) {
    *stride = (n_paths + 63) & ~int64_t(63);
    Buffer* slab = new_buffer(std::max<int64_t>(*stride, 64) * n_streams);
    slab->refs = 0;
    try { fill(slab->ptr); }
    catch (...) { slab->refs = 1; buffer_unref(slab); throw; }
    return slab;
}

// … and its n_steps · n_factors vectors as views into it, each with its place in the generation
void Engine::slab_views(Buffer* slab, int64_t stride, int n_steps, int n_factors, int64_t n_paths, fmhip_vec* out) {
    const uint32_t bm_id = next_bm_id_++;
    for (int64_t s = 0; s < (int64_t)n_steps * n_factors; ++s) {
        Buffer* v = new Buffer();
        v->ptr = slab->ptr + s * stride; v->cap = 0; v->refs = 1; v->parent = slab;
        slab->refs++;
        Node* nd = new_node(n_paths);
        nd->buf = v;
        nd->bm_id = bm_id; nd->bm_step = (int32_t)(s / n_factors); nd->bm_steps = n_steps;
        out[s] = nd->id;
    }
}

void Engine::bm_generate(int64_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                         const double* dt, fmhip_vec* out) {
    require_init(); check_n(n_paths);
    if (n_steps <= 0 || n_factors <= 0 || !dt || !out || path_offset < 0)
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad Brownian motion description");
    if (n_factors > 32768) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "more than 32768 factors");      // one launch keeps whole steps together (grid.y)
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    int64_t stride = 0;
    Buffer* slab = slab_generate(n_paths, n_streams, &stride, [&](float* vectors) {
        void* sq_dev = nullptr; size_t sq_cap = 0;
        try {
            float* st = (float*)ensure_stage((size_t)n_streams * 4);       // one entry per stream: the kernel reads it with a scalar load, no division
            for (int i = 0; i < n_steps; ++i) {
                if (!(dt[i] >= 0.0)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "negative time step");
                const float sq = (float)std::sqrt(dt[i]);                  // (float)Math.sqrt(timeStep), BrownianMotionCudaWithRandomVariableCuda.java:170
                for (int f = 0; f < n_factors; ++f) st[(size_t)i * n_factors + f] = sq;
            }
            sq_dev = pool_.alloc((size_t)n_streams * 4, &sq_cap);
            hip_check(hipMemcpyAsync(sq_dev, st, (size_t)n_streams * 4, hipMemcpyHostToDevice, stream_), "sqrt_dt H2D");
            hip_check(hipStreamSynchronize(stream_), "sync");
            if (n_paths > 0) {
                const int64_t chunk = 32768 - (32768 % n_factors);         // grid.y limit; keep whole steps together
                for (int64_t s0 = 0; s0 < n_streams; s0 += chunk) {
                    const int64_t ns = std::min(chunk, n_streams - s0);
                    DevBmArgs a{};
                    a.slab = vectors + s0 * stride;
                    a.sqrt_dt = (const float*)sq_dev + s0;
                    a.stride_floats = stride; a.n_paths = n_paths; a.path_offset = path_offset;
                    a.key0 = (uint32_t)(uint64_t)seed; a.key1 = (uint32_t)((uint64_t)seed >> 32);
                    a.n_factors = (uint32_t)n_factors; a.stream0 = (uint32_t)s0;
                    hipEvent_t ev0 = nullptr, ev1 = nullptr;            // fmhip_profile_enable: the generator's launches are bracketed like program launches
                    if (profiling_) { hip_check(hipEventCreate(&ev0), "hipEventCreate"); hip_check(hipEventCreate(&ev1), "hipEventCreate"); hip_check(hipEventRecord(ev0, stream_), "hipEventRecord"); }
                    hip_check(launch_bm(a, (uint32_t)ns, stream_), "launch fm_bm_kernel");
                    if (profiling_) { hip_check(hipEventRecord(ev1, stream_), "hipEventRecord"); profile_events_.push_back({ ev0, ev1 });
                                      profile_tags_.push_back({ 0, 0, (int)ns, 0, 1, 3, n_paths }); }
                    algorithmic_bytes_ += 4 * n_paths * ns;
                    bytes_written_ += 4 * n_paths * ns;
                    n_launches_++;
                }
            }
        } catch (...) {
            if (sq_dev) pool_.release(sq_dev, sq_cap);
            throw;
        }
        pool_.release(sq_dev, sq_cap);
    });
    slab_views(slab, stride, n_steps, n_factors, n_paths, out);
}

// ---------------------------------------------------------------- pool entry points

// (values that were left unstored are computed and stored first: their recipes may be all that keeps other vectors alive)
void Engine::pool_clean() { require_init(); if (has_late()) drain_late(); materialize_deferred(); hip_check(hipStreamSynchronize(stream_), "sync"); pool_.purge(); }

void Engine::pool_purge() {
    require_init();
    if (has_late()) drain_late();
    hip_check(hipStreamSynchronize(stream_), "sync");
    pool_.purge();
    for (auto& kv : plan_cache_) for (BigPlan::Seg& seg : kv.second.segs) { if (--seg.prog->refs == 0) delete seg.prog; delete seg.prog_red; }
    plan_cache_.clear();
    for (auto it = program_cache_.begin(); it != program_cache_.end();) { if (--it->second->refs == 0) delete it->second; it = program_cache_.erase(it); }
    schedule_cache_.clear(); schedule_cache_bytes_ = 0; dag_policies_.clear(); policy_reset();      // … and what was learnt about the shapes' handles
}

void Engine::engine_stats(fmhip_engine_stats_t* out) {
    require_init();
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "null stats pointer");
    std::memset(out, 0, sizeof *out);
    out->size = (int64_t)sizeof *out;
    out->kernel_launches = n_launches_; out->specialised_launches = n_jit_launches_; out->interpreter_launches = n_interpreter_launches_;
    out->algorithmic_bytes = algorithmic_bytes_; out->algorithmic_bytes_written = bytes_written_;
    out->values_deferred = n_deferred_total_; out->values_deferred_now = (int64_t)n_deferred_; out->values_demanded = n_demanded_;
    out->pending_operations = (int64_t)n_pending_;
    out->peak_bytes_reserved = pool_.peak_reserved;
    out->late_releases_while_waiting = n_late_waiting_; out->late_releases_at_once = n_late_at_once_; out->late_release_nanoseconds = late_ns_;
    out->merged_launches = n_merged_launches_; out->merged_chains = n_merged_chains_; out->common_rows = n_common_rows_;
    out->rolled_launches = n_rolled_launches_;
}

void Engine::pool_stats(fmhip_pool_stats_t* out) {
    require_init();
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "null stats pointer");
    if (has_late()) drain_late();
    size_t fr = 0, tot = 0;
    hip_check(hipMemGetInfo(&fr, &tot), "hipMemGetInfo");
    out->bytes_reserved = pool_.reserved; out->bytes_in_use = pool_.in_use; out->bytes_cached = pool_.cached;
    out->device_bytes_free = (int64_t)fr; out->device_bytes_total = (int64_t)tot;
    out->n_alloc_hits = pool_.hits; out->n_alloc_misses = pool_.misses;
    out->n_live_vectors = (int64_t)nodes_.size();
    out->n_kernel_launches = n_launches_; out->n_ops_executed = n_ops_executed_;
}

// ---------------------------------------------------------------- measurement

void Engine::profile_enable(bool on) {
    require_init();
    if (!on) { for (auto& p : profile_events_) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); } profile_events_.clear(); profile_tags_.clear(); }
    profiling_ = on;
}

void Engine::profile_read(double* ms_total, int64_t* n) {
    require_init();
    hip_check(hipStreamSynchronize(stream_), "sync");
    double total = 0.0;
    // FMHIP_PROFILE_DUMP=1: per program shape (ops/in/out/red/rows/tier), launches, device time and algorithmic GB/s
    const bool dump = std::getenv("FMHIP_PROFILE_DUMP") != nullptr;
    struct Agg { long long launches = 0; double ms = 0.0, bytes = 0.0; };
    std::map<std::string, Agg> agg;
    for (size_t i = 0; i < profile_events_.size(); ++i) {
        auto& p = profile_events_[i];
        float ms = 0.0f;
        hip_check(hipEventElapsedTime(&ms, p.first, p.second), "hipEventElapsedTime");
        total += ms;
        (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second);
        if (dump && i < profile_tags_.size()) {
            const ProfileTag& t = profile_tags_[i];
            char key[128];
            std::snprintf(key, sizeof key, "ops %3d in %2d out %d red %d rows %4d n %9lld %s", t.n_ops, t.n_in, t.n_out, t.n_red, t.batch, (long long)t.n, t.tier == 4 ? "merged chains" : t.tier == 3 ? "fm_bm_kernel" : t.tier ? "specialised" : "interpreter");
            Agg& a = agg[key];
            a.launches++; a.ms += ms; a.bytes += 4.0 * (double)t.n * (t.n_in + t.n_out) * t.batch;
        }
    }
    if (dump) {
        std::vector<std::pair<std::string, Agg>> v(agg.begin(), agg.end());
        std::sort(v.begin(), v.end(), [](const auto& a, const auto& b) { return a.second.ms > b.second.ms; });
        std::fprintf(stderr, "[fmhip profile] %zu launches, %.3f ms of kernel time\n", profile_events_.size(), total);
        for (const auto& kv : v)
            std::fprintf(stderr, "  %-72s %7lld launches %9.3f ms %8.1f us each %8.0f GB/s\n", kv.first.c_str(), kv.second.launches, kv.second.ms,
                         kv.second.ms / kv.second.launches * 1e3, kv.second.ms > 0 ? kv.second.bytes / (kv.second.ms * 1e-3) / 1e9 : 0.0);
    }
    profile_tags_.clear();
    if (ms_total) *ms_total = total;
    if (n) *n = (int64_t)profile_events_.size();
    profile_events_.clear();
}

} // namespace fm

#include "plans_engine.hpp"            // Engine::segment_dag, run_plan and its steps, plan_segments, run_big_group: components larger than one launch, from a group of one shape to launches
#include "loop_engine.hpp"             // Engine::detect_loop, plan_peel, plan_loop, run_rolled, run_peeled: the periodic stretch of a component as one launch
#include "merged_chains_engine.hpp"    // Engine::match_small, merge_shape_index, merge_families: components of one loop shape over the same vectors as one launch
#include "expectations_engine.hpp"     // Engine::red_*, arena_*, slot_wait, reduce, reduce_batch*, give_up_values, ticket_*: from a vector to its expectation
#include "side_pass_engine.hpp"        // Engine::pass_*: the frame the reducing passes below stand in
#include "order_stats_engine.hpp"      // Engine::os_*: the order-statistics passes
#include "cross_moments_engine.hpp"    // Engine::xmom_pass: the cross moments of a regression in one launch
#include "mt_generate_engine.hpp"      // Engine::mt_bm_generate, mt_increments_generate: finmath's Mersenne-Twister stream entered on the device
#include "sobol_engine.hpp"            // Engine::sobol_bm_generate: Sobol' points through a Brownian bridge
#include "binned_engine.hpp"           // Engine::binned_xmom_pass, binned_eval: the cross moments per bin of a key, the piecewise estimate
#include "xmom_wide_engine.hpp"        // Engine::xmom_wide_pass: the cross moments of up to 64 vectors in one launch on the matrix cores
#include "xmom_poly_engine.hpp"        // Engine::xmom_poly_pass, poly_eval: the same for a polynomial basis formed in registers, the fitted polynomial
#include "sort_engine.hpp"             // Engine::sort_by_key, argsort, rank_scores, read_elements: a stable radix sort of (key, path) pairs and what is made of its permutation
#include "prefix_engine.hpp"           // Engine::prefix_sums, prefix_sums_at, prefix_search: fp64 prefix sums in a tree that is a function of n alone
#include "resample_engine.hpp"         // Engine::resample: ancestors drawn from the cumulative weights, the state vectors gathered along
#include "select_engine.hpp"           // Engine::compress, expand, gather: the paths on which a mask is selected as shorter vectors, back again, and a gather by an index
#include "group_engine.hpp"            // Engine::group_sums: reduce by key — count, sum, mean and variance per group of an index vector
#include "table_engine.hpp"            // Engine::table_apply: tabulated functions of a vector's elements, a new vector each from one launch
#include "analytic_engine.hpp"         // Engine::function_apply, option_formula: Φ, φ, Φ⁻¹ and the Black–Scholes / Bachelier formulas per path
#include "implied_volatility_engine.hpp"      // Engine::implied_volatility: the inverse of the option formulas' value in the volatility, per path
#include "transform_engine.hpp"               // Engine::transform_option: a call under an exponential-affine transform as a sum over a node table, per path
#include "kreg_engine.hpp"             // Engine::kernel_moments_pass: kernel-weighted local moments at a grid of points of a key in one launch
#include "nested_engine.hpp"           // Engine::block_moments, repeat: the moments of consecutive blocks as new vectors, k inner paths per outer state
#include "block_order_engine.hpp"      // Engine::block_order_statistics, block_sort: ranks and range means of consecutive blocks as new vectors, the blocks sorted
#include "cross_order_engine.hpp"      // Engine::cross_order_statistics, cross_select: ranks of the K values of every path as values and slots, the element an index names
