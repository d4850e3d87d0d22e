// side_pass_engine.hpp — the frame of the engine's side passes: a kernel of its own beside the lazy graph that leaves a few numbers in
// pinned memory (the REDUCING passes: order_stats_engine.hpp, cross_moments_engine.hpp, binned_engine.hpp …) or new, materialised vectors
// (the PRODUCING passes: table_engine.hpp, analytic_engine.hpp, nested_engine.hpp, sort_engine.hpp, prefix_engine.hpp and the evaluations
// of binned_engine.hpp and xmom_poly_engine.hpp).  Part of runtime.cpp's translation unit (included at its end, before the passes, nowhere
// else): Engine member functions in a file of their own because runtime.cpp is long enough, and in that translation unit so that every
// build that lists the engine's sources — the library's, the sanitizer builds against the null device — has them without being told.
//
// A pass: checks its arguments (pass_size among them) before anything is flushed or launched, refuses a build without its kernel
// (pass_need_kernel: FMHIP_ERR_UNSUPPORTED — the mirrors' host path is a caller's choice, never the engine's), ends a step group, counts as
// a use of every vector (escape policy), computes what is pending or deferred below the batch in ONE flush, takes a reference on every
// vector's STORAGE and forgets the nodes (pass_prepare) — the wait that follows may not rely on a Node* (queued releases are not performed
// during it either: it polls the flag and falls back to the plain stream wait) —, lays out its pinned block as [tables the launch reads]
// [what it writes] [flag] and its device scratch (pass_scratch), launches once and waits under the engine lock as read() does (pass_launch;
// pass_launch_raising where the chain ends in the one-lane kernel that raises the flag).  Shared storage (common rows) is only read.
// `what` names the pass in whatever the frame has to say.
//
// A producing pass allocates its outputs through PassOutputs behind pass_prepare and BEFORE anything is staged or launched — an allocation
// that fails leaves nothing copied or launched — and ends in PassOutputs::commit, the one place that writes a caller's handle: a refusal at
// any stage leaves `out` untouched, no vector and no byte behind.
#include "runtime.hpp"
#include "pinned_wait.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace fm {

// The passes' launchers are WEAK references: a host-only build of the engine whose stand-in for the kernels does not know one
// (tests/nulldev/null_hip.cpp; null_os.cpp, null_xmom.cpp and null_binned.cpp add them) still links.  Calling one that is missing is an
// error — there is no fallback: the mirrors' host path is a caller's choice, never the engine's.
static void pass_need_kernel(bool present, const char* what) {
    if (!present) throw Error(FMHIP_ERR_UNSUPPORTED, std::string("this build of the engine has no ") + what + " kernel");
}

static size_t pass_up256(size_t b) { return (b + 255) & ~size_t(255); }

// the host definitions and argument rules (host/*.hpp) complain with std::invalid_argument: the same complaint as an engine error
template <class F> static void pass_as_engine_error(F&& f) {
    try { f(); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}

// the one-lane kernel that raises the flag behind a chain of launches (sort_kernel.hip); WEAK like every launcher of a pass
hipError_t launch_sort_done(uint64_t* done_flag, uint64_t done_value, hipStream_t st) __attribute__((weak));

struct Engine::PassHold {          // the storage of a batch, referenced for the duration of a pass
    Engine* e = nullptr;
    std::vector<Buffer*> held;
    std::vector<uint64_t> ptrs;
    int64_t n = 0;
    ~PassHold() { for (Buffer* b : held) e->buffer_unref(b); }
};

struct Engine::PassOutputs {       // the freshly allocated outputs of a producing pass: back in the pool unless the pass commits them
    struct Slot { Buffer* b; int64_t n; fmhip_vec id; };
    Engine* e;
    std::vector<Slot> slots;
    bool committed = false;
    explicit PassOutputs(Engine* eng) : e(eng) {}
    PassOutputs(const PassOutputs&) = delete;
    ~PassOutputs() { for (Slot& s : slots) { if (s.b) e->buffer_unref(s.b); else if (s.id && !committed) e->release(s.id); } }
    uint64_t add(int64_t n_floats) {
        slots.push_back({ nullptr, n_floats, 0 });             // the slot first: nothing can throw between an allocation and its guard
        slots.back().b = e->new_buffer(n_floats);
        return (uint64_t)(uintptr_t)slots.back().b->ptr;
    }
    // One node per buffer, in the order of allocation; the handles are written when every node exists: first, if given, receives the first
    // one, out the others.  A new_node that throws half-way writes nothing: the nodes made so far own their buffers and are released with
    // them, the other buffers are given back (~PassOutputs).
    void commit(fmhip_vec* out, fmhip_vec* first = nullptr) {
        for (Slot& s : slots) { Node* nd = e->new_node(s.n); nd->buf = s.b; s.b = nullptr; s.id = nd->id; }
        committed = true;
        size_t k = 0;
        if (first) *first = slots[k++].id;
        for (; k < slots.size(); ++k) *out++ = slots[k].id;
    }
};

// hs: the handles of a pass that have a node (the constant 1, handle 0 among the x of a regression, has none and no size: its callers leave it out)
int64_t Engine::pass_size(const fmhip_vec* hs, int count, const char* what) {
    require_init();
    if (!hs || count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + " of no vector");
    const int64_t n = node(hs[0])->n;
    for (int i = 1; i < count; ++i)
        if (node(hs[i])->n != n) throw Error(FMHIP_ERR_SIZE_MISMATCH, std::string(what) + " over vectors of different size");
    if (n <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + " of an empty vector");
    return n;
}

void Engine::pass_prepare(const fmhip_vec* hs, int count, PassHold& hold, const char* what) {
    hold.e = this;
    hold.n = pass_size(hs, count, what);
    if (count > 65535) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string("more than 65535 vectors in one ") + what + " call");
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

void Engine::pass_scratch(size_t zero_bytes, size_t other_bytes) {
    auto grow = [&](void*& p, size_t& cap, size_t need, bool zero) {
        if (need <= cap && !(zero && pass_dirty_)) return;
        if (need > cap) {
            if (p) { hip_check(hipStreamSynchronize(stream_), "sync"); (void)hipFree(p); p = nullptr; cap = 0; }
            const size_t c = std::max(pass_up256(need), size_t(1) << 16);
            hip_check(hipMalloc(&p, c), "hipMalloc(side pass scratch)");
            cap = c;
        }
        if (zero) hip_check(hipMemsetAsync(p, 0, cap, stream_), "hipMemsetAsync(side pass scratch)");
    };
    grow(pass_zero_, pass_zero_cap_, zero_bytes, true);
    pass_dirty_ = false;
    grow(pass_other_, pass_other_cap_, other_bytes, false);
}

void Engine::pass_release() {
    if (pass_zero_) (void)hipFree(pass_zero_);
    if (pass_other_) (void)hipFree(pass_other_);
    pass_zero_ = pass_other_ = nullptr; pass_zero_cap_ = pass_other_cap_ = 0; pass_dirty_ = false;
}

void Engine::pass_wait(volatile uint64_t* flag, uint64_t value, const char* what) {
    bool arrived = spin_until([&] { return *flag == value; }, [] { pause(); });
    if (!arrived) { hip_check(hipStreamSynchronize(stream_), "side pass sync"); arrived = *flag == value; std::atomic_thread_fence(std::memory_order_acquire); }
    if (!arrived) throw Error(FMHIP_ERR_HIP, std::string("the ") + what + " ended without delivering its results");
    pass_dirty_ = false;
}

// The armed launch.  `flag`: the last word of the pass's pinned block; done_flag, done_value: where the launch's arguments want it and the
// value it receives; launch(): the launcher's status.  The zero scratch counts as dirty until the flag has arrived: a launch that fails
// half-way leaves counters behind, and the next pass clears them (pass_scratch).
template <class Launch>
inline void Engine::pass_launch(volatile uint64_t* flag, uint64_t*& done_flag, uint64_t& done_value, const char* what, Launch launch) {
    done_flag = const_cast<uint64_t*>(flag); done_value = ++pass_seq_;
    *flag = 0;
    pass_dirty_ = true;
    hip_check(launch(), what);
    ++n_launches_;
    pass_wait(flag, done_value, what);
}

// The same for a chain that knows no flag: enqueue(), then the one-lane kernel that raises it.
template <class Enqueue>
inline void Engine::pass_launch_raising(volatile uint64_t* flag, const char* what, Enqueue enqueue) {
    uint64_t* done_flag = nullptr; uint64_t done_value = 0;
    pass_launch(flag, done_flag, done_value, what, [&] {
        hipError_t e = enqueue();
        if (e == hipSuccess) e = launch_sort_done(done_flag, done_value, stream_);
        return e;
    });
}

} // namespace fm
