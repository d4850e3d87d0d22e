// expectations_engine.hpp — everything between a vector and its expectation: what a launch with fused reductions holds and how its
// moments are waited for (red_*), the pinned arena whose slots receive the moments that launches take along without being waited for
// (arena_*, slot_*), the reductions themselves (reduce, reduce_batch and its ticket and device-buffer forms, give_up_values) and the
// tickets (ticket_*).  Part of runtime.cpp's translation unit (included at its end, before side_pass_engine.hpp, nowhere else): Engine
// member functions in a file of their own because runtime.cpp is long enough, and in that translation unit so that every build that lists
// the engine's sources — the library's, the sanitizer builds against the null device — has them without being told.
//
// Every wait for a word of pinned memory in here is ONE loop, spin_until (pinned_wait.hpp: its comment has the table of who does what
// between two looks and after a timeout); every rule of the batched forms — the nodes of a batch and their one size (batch_nodes), when the
// flush takes the moments along (from_launches_applies, flush_for_moments, Engine::MomentsAlong), what is left for ONE reduction launch
// afterwards (moments_missing) — is written once.
#include "runtime.hpp"
#include "pinned_wait.hpp"

#include <algorithm>
#include <cstring>
#include <thread>

namespace fm {

// ---------------------------------------------------------------- the pinned arena and its slots

double* Engine::arena_alloc(size_t count)
{
    const size_t need = count * 32;
    if (need > ARENA_BYTES) return nullptr;
    if (arena_off_ + need > ARENA_BYTES) {                     // full: everything written so far is collected, then it starts again
        wait_for_stream("hipStreamSynchronize(moments arena)");
        arena_collect();
        arena_off_ = 0;
    }
    volatile uint64_t* p = reinterpret_cast<volatile uint64_t*>(moments_arena_ + arena_off_);
    for (size_t i = 0; i < count * 4; ++i) p[i] = MOMENTS_SENTINEL;
    arena_off_ += need;
    return reinterpret_cast<double*>(const_cast<uint64_t*>(p));
}

void Engine::arena_assign(Node* nd, double* slot)
{
    nd->has_moments = false;
    nd->moments_slot = reinterpret_cast<volatile uint64_t*>(slot);
    arena_outstanding_.push_back({ nd->id, nd->moments_slot });
}

// The moments a launch takes along for its roots (runtime.hpp): arena slots in a flush that does not wait, else a host array.
bool Engine::RootMoments::open(Engine& engine, size_t count)
{
    e = &engine;
    if (engine.async_moments_) slots = engine.arena_alloc(count); else all.resize(count);
    return is_open();
}

void Engine::RootMoments::deliver(Node* root, size_t slot)
{
    if (slots) e->arena_assign(root, slots + slot * 4); else set_moments(root, all[slot]);
}

bool Engine::slot_arrived(const volatile uint64_t* slot)
{
    return slot[0] != MOMENTS_SENTINEL && slot[1] != MOMENTS_SENTINEL && slot[2] != MOMENTS_SENTINEL && slot[3] != MOMENTS_SENTINEL;
}

void Engine::slot_take(const volatile uint64_t* slot, void* out32)
{
    const uint64_t v[4] = { slot[0], slot[1], slot[2], slot[3] };
    std::memcpy(out32, v, 32);
}

void Engine::arena_collect()
{
    for (const auto& o : arena_outstanding_) {
        Node* nd = nodes_.get(o.first);
        if (!nd || nd->moments_slot != o.second) continue;       // gone, asked for already, or written into since
        nd->moments_slot = nullptr;
        if (slot_arrived(o.second)) { slot_take(o.second, nd->moments); nd->has_moments = true; }
    }
    arena_outstanding_.clear();
    for (auto& kv : tickets_) {                                   // tickets that wait for slots: what they wait for has arrived
        MomentsTicket& t = kv.second;
        for (size_t i = 0; i < t.slots.size(); ++i)
            if (volatile uint64_t* slot = t.slots[i]) { slot_take(slot, &t.ready[i]); t.slots[i] = nullptr; }
    }
}

void Engine::drain_or_pause()
{
    if (has_late()) drain_late(late_portion());           // the device is being waited for: queued releases are performed meanwhile, a few per look
    else pause();
}

bool Engine::slot_wait(Node* nd)
{
    volatile uint64_t* slot = nd->moments_slot;
    if (!slot) return false;
    bool arrived = spin_until([&] { return slot_arrived(slot); }, [&] { drain_or_pause(); });
    if (!arrived) { wait_for_stream("moments sync"); arrived = slot_arrived(slot); std::atomic_thread_fence(std::memory_order_acquire); }
    nd->moments_slot = nullptr;
    if (!arrived) return false;                                  // (the launch never took them: a failed launch)
    slot_take(slot, nd->moments);
    nd->has_moments = true;
    return true;
}

// ---------------------------------------------------------------- a launch with fused reductions

// The buffers a launch with fused reductions needs, and where its moments go.  Results wanted on the host only: the last workgroup of
// a row stores its 32 bytes straight into the pinned staging buffer (host memory is mapped into the device's address space) — no
// device-to-host copy command between the kernel and the wait (a `chain.getAverage()` through the C++ mirror at 100 / 5 000 paths:
// 19.6 → 17.7 / 22.9 → 21.2 µs, benchmarks/small_n_latency.cpp).  One row, results wanted on the host: the kernel raises a flag in
// pinned memory behind the results and the host POLLS it instead of synchronising the stream.  A caller that values one product after
// the other (finmath-lib's calibration: 144 getAverage() per objective evaluation) pays the wake-up of hipStreamSynchronize and,
// measured, a launch that takes 20–25 µs instead of 5 right after it, once per product.
void Engine::red_begin(RedLaunch& red, int batch, int n_red, size_t blocks_per_row, fmhip_moments* host_moments, void* dev_moments)
{
    red = RedLaunch();
    red.dev_moments = dev_moments;
    red.on_host = host_moments && !dev_moments;
    red.partials = pool_.alloc((size_t)batch * n_red * (blocks_per_row + 8) * 32, &red.partials_cap);       // + FM_COMBINE_GROUP_SLOTS group partials per row
    static const bool POLL = knob_on("FMHIP_POLL");
    try {
        if (dev_moments) red.results = dev_moments;
        else if (red.on_host && POLL && batch == 1 && n_red <= 2 && !free_slots_.empty()) {       // a slot of its own: results [0, 64), flag at 64
            red.slot = free_slots_.back(); free_slots_.pop_back();
            red.results = result_slots_ + (size_t)red.slot * 128;
        }
        else if (red.on_host) red.results = ensure_stage((size_t)batch * n_red * 32);
        else red.results = pool_.alloc((size_t)batch * n_red * 32, &red.results_cap);
    } catch (...) { pool_.release(red.partials, red.partials_cap); red.partials = nullptr; throw; }
    if (red.slot >= 0) {
        red.poll_flag = reinterpret_cast<volatile uint64_t*>((char*)red.results + 64);
        *red.poll_flag = 0;
        red.done_value = ++poll_sequence_;
    }
}

bool Engine::red_poll(const RedLaunch& red)
{
    if (!red.poll_flag) return false;
    return spin_until([&] { return *red.poll_flag == red.done_value; }, [] { pause(); });      // a long kernel: wait the ordinary way
}

void Engine::red_complete(RedLaunch& red, bool arrived)
{
    if (!red.pending) return;
    red.pending = false;
    try {
        if (!arrived) wait_for_stream("moments sync");
        std::memcpy(red.host, red.results, (size_t)red.batch * red.n_red * 32);
    } catch (...) { red_release(red); throw; }
    red_release(red);
}

void Engine::red_wait(RedLaunch& red, int batch, int n_red, fmhip_moments* host_moments)
{
    if (!host_moments) return;
    const size_t bytes = (size_t)batch * n_red * 32;
    void* src = red.results;
    if (!red.on_host) { src = ensure_stage(bytes); hip_check(hipMemcpyAsync(src, red.results, bytes, hipMemcpyDeviceToHost, stream_), "moments D2H"); }
    bool arrived = false;
    if (red.poll_flag && has_late())                        // (as red_poll, with queued releases performed between the looks)
        arrived = spin_until([&] { return *red.poll_flag == red.done_value; }, [&] { if (has_late()) drain_late(late_portion()); }, 64);
    if (!arrived && !red_poll(red)) wait_for_stream("moments sync");
    std::memcpy(host_moments, src, bytes);
}

void Engine::red_release(RedLaunch& red)
{
    if (red.partials) pool_.release(red.partials, red.partials_cap);
    if (red.results && !red.dev_moments && !red.on_host) pool_.release(red.results, red.results_cap);
    if (red.slot >= 0) { free_slots_.push_back(red.slot); red.slot = -1; }
    red.partials = nullptr; red.results = nullptr; red.poll_flag = nullptr;
}

// ---------------------------------------------------------------- reductions

// The stand-alone reduction is the empty program with one fused reduction of its input (compiled once).
Program* Engine::reduce_program() {
    static const char* key = "__reduce1";
    auto it = program_cache_.find(key);
    if (it != program_cache_.end()) return it->second;
    Program* prog = compile({}, 1, {}, { 0 }, nullptr, true);
    if (jit_mode != FMHIP_JIT_OFF) prog->jit = jit().request(prog->proto, jit_mode == FMHIP_JIT_SYNC);      // every getAverage() runs it: specialised from the start (it is in the kernel pack)
    program_cache_[key] = prog;
    return prog;
}

void Engine::reduce(fmhip_vec h, double shift, fmhip_moments* host_out, void* dev_out, RedLaunch* hand_over) {
    require_init();
    end_step_group();
    Node* nd = node(h);
    auto cached = [&]() {
        if (!(nd->has_moments && shift == 0.0 && host_out && !dev_out)) return false;
        *host_out = moments_of(nd);
        return true;
    };
    if (cached()) return;
    if (nd->moments_slot && shift == 0.0 && host_out && !dev_out && slot_wait(nd) && cached()) return;
    ++flush_seq_;
    // One expectation is asked for while much else is pending (a caller that records the payoffs of all its products and then takes
    // their averages one by one — 144 per objective evaluation of the LIBOR market model calibration): everything pending runs NOW,
    // components of equal shape as rows of the same launches, and those launches take the moments of their roots along.  The other
    // products' getAverage() calls are answered from what is left with their nodes; the moments are those of the stand-alone
    // reduction to the last bit (one reduction tree per vector: fm_kernel_parts.hpp).
    static const size_t BATCH_PENDING = knob_size("FMHIP_BATCH_EXPECTATIONS", (size_t)256);   // 0 = off
    if (BATCH_PENDING && fusion && fusion_hold != 1 && !nd->buf && shift == 0.0 && host_out && !dev_out && n_pending_ >= BATCH_PENDING && n_pending_ >= 4 * (size_t)std::max(1, nd->weight)) {
        MomentsAlong along(this, false);
        flush_all();
    }
    if (cached()) return;
    if (nd->moments_slot && shift == 0.0 && host_out && !dev_out && slot_wait(nd) && cached()) return;
    touch(nd);
    RedLaunch deferred;
    struct Defer {                      // the launch that takes the moments hands its wait to this scope (RedLaunch::pending)
        Engine* e; RedLaunch* r; RedLaunch* hand_over;
        Defer(Engine* e_, RedLaunch* r_, RedLaunch* h_) : e(e_), r(r_), hand_over(h_) { e->defer_red_ = r; }
        ~Defer() { e->defer_red_ = nullptr; if (r->pending) { r->pending = false; (void)hipStreamSynchronize(e->stream_); e->red_release(*r); } }      // (an error behind the launch: its buffers go back when it has finished)
        // the moments: waited for here, or — results in a slot of their own, a caller that can wait without the engine lock — by the caller
        void finish() {
            e->defer_red_ = nullptr;
            if (!r->pending) return;
            if (hand_over && r->slot >= 0) { *hand_over = *r; r->pending = false; return; }
            e->red_wait(*r, r->batch, r->n_red, r->host); r->pending = false; e->red_release(*r);
        }
    } defer(this, &deferred, hand_over);
    if (!nd->buf) {
        // `chain.getAverage()`: the expectation of a pending expression that fits one launch is taken in THAT launch (the kernel's
        // fused reduction) instead of a second launch that reads the vector again — one launch and 4 B per path less.  A launch with a
        // fused reduction of a large row has one workgroup per 8192 elements (fine for a chain over two vectors, a starved launch for one
        // over eleven) unless it is small enough to take one UNIT of the reduction tree per workgroup (unit_launch).
        expand_replicas_below({ nd });
        std::vector<Dag> one(1);
        if (fusion && nd->weight <= 4 * FM_MAX_OPS && build_dag({ nd }, one[0]) && (nd->n * (int64_t)one[0].leaves.size() <= (int64_t(1) << 21) || unit_launch(nd->n, 1)) && run_dags(one, &shift, host_out, dev_out)) { defer.finish(); return; }
        // … and of one that takes several launches, in the LAST of them (when its plan exists: from the second time a shape is seen)
        if (fusion && !nd->buf && nd->n > 0) {
            std::vector<BigDag> big(1);
            if (build_big({ nd }, big[0])) {
                ReduceRequest rr{ shift, host_out, dev_out, false };
                run_big_group(big, &rr);
                if (rr.done) { defer.finish(); return; }
            }
        }
        defer.finish();
        defer_red_ = &deferred;
        if (!nd->buf) materialize({ nd });
    }
    Program* prog = reduce_program();
    std::vector<RowSpec> rows(1);
    rows[0].in.push_back(nd->buf->ptr);
    rows[0].scalars = nullptr;
    rows[0].shifts = &shift;
    launch(prog, nd->n, rows, host_out, dev_out);
    defer.finish();
}

std::vector<Node*> Engine::batch_nodes(const fmhip_vec* hs, int count) {
    std::vector<Node*> nds((size_t)count);
    for (int i = 0; i < count; ++i) nds[(size_t)i] = node(hs[i]);
    for (int i = 1; i < count; ++i)
        if (nds[(size_t)i]->n != nds[0]->n) throw Error(FMHIP_ERR_SIZE_MISMATCH, "batched reduction over vectors of different size");
    return nds;
}

void Engine::reduce_batch(const fmhip_vec* hs, int count, const double* shifts, fmhip_moments* host_out, void* dev_out) {
    HostTimer timer(HostProfile::REDUCE);
    require_init();
    end_step_group();
    if (count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "count must be positive");
    const std::vector<Node*> nds = batch_nodes(hs, count);
    bool pending = false;
    for (Node* nd : nds) { touch(nd); pending |= !nd->buf; }
    if (pending) flush_all();                                   // one batched flush instead of one launch per vector
    for (Node* nd : nds) if (!nd->buf) materialize({ nd });
    Program* prog = reduce_program();
    const int max_rows = (int)MAX_LAUNCH_ROWS;
    for (int off = 0; off < count; off += max_rows) {
        const int m = std::min(max_rows, count - off);
        std::vector<RowSpec> rows((size_t)m);
        for (int i = 0; i < m; ++i) {
            rows[(size_t)i].in.push_back(nds[(size_t)(off + i)]->buf->ptr);
            rows[(size_t)i].scalars = nullptr;
            rows[(size_t)i].shifts = shifts ? &shifts[off + i] : nullptr;
        }
        launch(prog, nds[0]->n, rows, host_out ? host_out + off : nullptr, dev_out ? (char*)dev_out + (size_t)off * 32 : nullptr);
    }
}

// The batched forms may leave the moments to the launches that compute the vectors: the knob (FMHIP_MOMENTS_FROM_LAUNCHES=0: off), fusion
// on, no shift.
bool Engine::from_launches_applies(int count, const double* shifts) const {
    static const bool FROM_LAUNCHES = knob_on("FMHIP_MOMENTS_FROM_LAUNCHES");
    bool unshifted = true;
    for (int i = 0; shifts && i < count; ++i) unshifted &= shifts[i] == 0.0;
    return FROM_LAUNCHES && fusion && unshifted;
}

void Engine::flush_for_moments(const std::vector<Node*>& nds) {
    bool pending = false;
    for (const Node* nd : nds) pending |= !nd->buf && !nd->discarded;
    if (!pending) return;
    MomentsAlong along(this, true);
    flush_all();
}

// What has neither moments nor a slot after the flush (computed earlier, a launch that could not take them along, a vector somebody
// writes into): it goes through ONE launch of the reduction program.
struct MomentsMissing { std::vector<fmhip_vec> handles; std::vector<size_t> index; };
static MomentsMissing moments_missing(const fmhip_vec* hs, const std::vector<Node*>& nds) {
    MomentsMissing rest;
    for (size_t i = 0; i < nds.size(); ++i)
        if (!nds[i]->has_moments && !nds[i]->moments_slot) { rest.handles.push_back(hs[i]); rest.index.push_back(i); }
    return rest;
}

int64_t Engine::reduce_batch_begin(const fmhip_vec* hs, int count, const double* shifts) {
    require_init();
    if (count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "count must be positive");
    // Vectors that are still pending: the flush that computes them takes their moments along (rows of the launches that compute them
    // anyway, results into slots of the pinned arena) — no reduction launch, the vectors are not read again.  The ticket remembers the
    // slots; ending it waits for them.  (Vectors computed already, shifts, or a component whose launches cannot take moments: the
    // reduction launch below.)
    if (from_launches_applies(count, shifts) && hs) return reduce_batch_begin_from_launches(hs, count);
    const size_t bytes = (size_t)count * 32;
    MomentsTicket t;
    for (size_t i = 0; i < free_tickets_.size(); ++i)
        if (free_tickets_[i].cap >= bytes) { t = free_tickets_[i]; free_tickets_[i] = free_tickets_.back(); free_tickets_.pop_back(); break; }
    try {
        if (!t.host) {
            t.cap = std::max(bytes, size_t(8192));
            hip_check(hipHostMalloc(&t.host, t.cap, hipHostMallocDefault), "hipHostMalloc(moments ticket)");
            hip_check(hipEventCreateWithFlags(&t.event, hipEventDisableTiming), "hipEventCreate(moments ticket)");
        }
        t.count = count;
        reduce_batch(hs, count, shifts, nullptr, t.host);     // the last workgroup of every row stores its moments straight into the block
        hip_check(hipEventRecord(t.event, stream_), "hipEventRecord(moments ticket)");
    } catch (...) { if (t.host) free_tickets_.push_back(t); throw; }
    const int64_t id = next_ticket_++;
    tickets_[id] = t;
    return id;
}

// fmhip_vec_give_up_values: the caller wants the EXPECTATIONS of these vectors and will never read their values.  A vector that is
// still pending and that nobody but the caller references is marked (Node::discard); a flush that takes the moments of its roots along
// (reduce_batch_begin, reduce) then computes it in a launch that takes its moments and does NOT store it (run_plan: a peeled component
// whose root is 'm' in the signature).  One 8 KB store per workgroup at the end of a read-only chain costs such a launch 8-10 % of its
// rate (benchmarks/read_pattern.hip: 6486 → 5893 GB/s; the valuation kernel in isolation 6145 → 6617): the memory system pays for
// turning a stream of reads around for a trickle of writes.  A marked vector that runs through a launch which cannot take its moments
// is stored like any other.
void Engine::give_up_values(const fmhip_vec* hs, int count) {
    require_init();
    if (count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "count must be positive");
    static const bool DISCARD = knob_on("FMHIP_DISCARD_VALUES");      // =0: every value is stored (A/B measurement)
    std::vector<Node*> nds((size_t)count);
    for (int i = 0; i < count; ++i) nds[(size_t)i] = node(hs[i]);
    if (!DISCARD) return;
    // nobody but the caller references it — not counting the holds of a live replica description (fmhip_graph_clone) on the roots it
    // replicates (one external reference on the original's root) and on the roots of its copies (one internal reference each)
    auto sole_owner = [&](const Node* nd) {
        int ext = nd->refs_ext, in = nd->refs_int;
        if (nd->rep_id && replica_of(nd)) { if (nd->rep_copy) in -= 1; else if (nd->rep_root >= 0) ext -= 1; }
        return ext == 1 && in == 0;
    };
    for (Node* nd : nds) if (!nd->buf && !nd->moments_blocked && sole_owner(nd)) nd->discard = true;
}

// The expectations of vectors that may still be pending, every one through a slot of the pinned arena (or at hand already): the flush
// that computes the pending ones takes their moments along; what has none afterwards (computed earlier, a launch that could not take
// them along, a vector somebody writes into) is reduced by ONE launch of the reduction program into arena slots.
int64_t Engine::reduce_batch_begin_from_launches(const fmhip_vec* hs, int count) {
    end_step_group();
    const std::vector<Node*> nds = batch_nodes(hs, count);
    flush_for_moments(nds);
    const MomentsMissing rest = moments_missing(hs, nds);
    MomentsTicket t;
    t.count = count; t.slots.resize((size_t)count, nullptr); t.ready.resize((size_t)count);
    if (!rest.handles.empty()) {
        double* slots = arena_alloc(rest.handles.size());
        if (!slots) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "too many expectations for one ticket");
        reduce_batch(rest.handles.data(), (int)rest.handles.size(), nullptr, nullptr, slots);
        for (size_t k = 0; k < rest.index.size(); ++k) t.slots[rest.index[k]] = reinterpret_cast<volatile uint64_t*>(slots + k * 4);
    }
    for (int i = 0; i < count; ++i) {
        Node* nd = nds[(size_t)i];
        if (t.slots[(size_t)i]) continue;
        if (nd->has_moments) t.ready[(size_t)i] = moments_of(nd);
        else t.slots[(size_t)i] = nd->moments_slot;
    }
    const int64_t id = next_ticket_++;
    tickets_[id] = std::move(t);
    return id;
}

// fmhip_reduce_moments_batch_device on vectors that may still be pending: as reduce_batch_begin_from_launches — the flush that computes them
// takes their moments along (values that were given up are not stored at all) — but the caller wants the 32-byte blocks in ONE device
// buffer, in the order asked (the send buffer of its RCCL exchange), not on the host: a one-wave kernel behind the launches collects them
// from their slots of the pinned arena, which the device reads through the same mapping it wrote them through.  Until round 4 a caller
// with a communicator of its own (lmm_hip --world N) had to flush first and pay a reduction launch that read every value again.
void Engine::reduce_batch_device_from_launches(const fmhip_vec* hs, int count, void* dev_out) {
    end_step_group();
    const std::vector<Node*> nds = batch_nodes(hs, count);
    flush_for_moments(nds);
    // one block of the arena for whatever has no slot yet, taken BEFORE the vectors are sorted: if the arena wraps here, the slots written so
    // far are collected into their nodes (has_moments) now and not between two looks at them
    double* block = arena_alloc((size_t)count);
    if (!block) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "too many expectations for one call");
    const MomentsMissing rest = moments_missing(hs, nds);
    std::vector<uint64_t> src((size_t)count, 0);
    size_t used = 0;
    for (int i = 0; i < count; ++i) {
        Node* nd = nds[(size_t)i];
        if (nd->moments_slot) src[(size_t)i] = (uint64_t)(uintptr_t)nd->moments_slot;
        else if (nd->has_moments) { double* at = block + 4 * used++; std::memcpy(at, nd->moments, 32); src[(size_t)i] = (uint64_t)(uintptr_t)at; }
    }
    if (!rest.handles.empty()) {   // computed earlier, or by a launch that could not take the moments along: one reduction launch, into the block
        double* at = block + 4 * used;
        reduce_batch(rest.handles.data(), (int)rest.handles.size(), nullptr, nullptr, at);
        for (size_t k = 0; k < rest.index.size(); ++k) src[rest.index[k]] = (uint64_t)(uintptr_t)(at + 4 * k);
        used += rest.handles.size();
    }
    { volatile uint64_t* tail = reinterpret_cast<volatile uint64_t*>(block + 4 * used); for (size_t i = 0; i < ((size_t)count - used) * 4; ++i) tail[i] = 0; }    // (unused slots: no sentinels left behind)
    for (int off = 0; off < count; off += FM_GATHER_MAX) {
        DevGatherArgs a{};
        a.count = (uint32_t)std::min(FM_GATHER_MAX, count - off);
        std::memcpy(a.src, src.data() + off, (size_t)a.count * 8);
        hip_check(launch_gather_moments(a, (double*)dev_out + (size_t)off * 4, stream_), "launch fm_gather_moments_kernel");
        n_launches_++;
    }
}

void Engine::reduce_batch_device(const fmhip_vec* hs, int count, const double* shifts, void* dev_out) {
    require_init();
    if (count <= 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "count must be positive");
    bool worth = false;                                          // something is pending, given up, or has its moments already
    if (from_launches_applies(count, shifts)) for (int i = 0; i < count && !worth; ++i) { const Node* nd = node(hs[i]); worth = !nd->buf || nd->has_moments || nd->moments_slot; }
    if (worth) reduce_batch_device_from_launches(hs, count, dev_out);
    else reduce_batch(hs, count, shifts, nullptr, dev_out);
}

// ---------------------------------------------------------------- tickets

Engine::MomentsTicket Engine::ticket_take(int64_t id) {
    auto it = tickets_.find(id);
    if (it == tickets_.end()) throw Error(FMHIP_ERR_INVALID_HANDLE, "unknown (or already ended) expectation ticket");
    MomentsTicket t = std::move(it->second);
    tickets_.erase(it);
    for (size_t i = 0; i < t.slots.size(); ++i) {                 // moments taken by the launches that computed the vectors: wait for their slots
        volatile uint64_t* slot = t.slots[i];
        if (!slot) continue;
        bool arrived = spin_until([&] { return slot_arrived(slot); }, [&] { drain_or_pause(); });
        // Not there after 2 ms of spinning: the launch that writes it is far down the queue.  Keep watching THIS slot, asleep in between —
        // never hipStreamSynchronize: that waits for everything queued behind as well (a driver that records batch b+1 before it asks
        // for batch b's expectations lost its overlap at every second batch that way: the device drained, then idled 2 ms per batch
        // while the host recorded the next one).  A stream that has run dry without the slot being written is an error.
        for (uint32_t naps = 1; !arrived; ++naps) {
            std::this_thread::sleep_for(std::chrono::microseconds(50));
            arrived = slot_arrived(slot);
            if (!arrived && (naps & 63u) == 0) {
                const hipError_t q = hipStreamQuery(stream_);
                if (q == hipSuccess) { arrived = slot_arrived(slot); break; }
                if (q != hipErrorNotReady) hip_check(q, "hipStreamQuery(moments)");
            }
        }
        if (!arrived) throw Error(FMHIP_ERR_HIP, "the moments of a vector never arrived");
        std::atomic_thread_fence(std::memory_order_acquire);
        slot_take(slot, &t.ready[i]);
        t.slots[i] = nullptr;
    }
    return t;
}

void Engine::ticket_retire(MomentsTicket& t) {
    t.slots.clear(); t.ready.clear();
    if (t.host) free_tickets_.push_back(t);
    t = MomentsTicket();
}

} // namespace fm
