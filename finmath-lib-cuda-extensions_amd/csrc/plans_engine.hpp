// plans_engine.hpp — components larger than one launch, from "a group of components of one shape" to launches: the segment of a
// component as a Dag (segment_dag), a planned segment over a group (run_planned_segment), a shape's plan over a group (run_plan, a
// driver over named steps), the cutting of a shape on first use (plan_segments: cuts are committed WHOLE) and the entry, run_big_group.
// build_big, which makes the components, and the flush, which groups them, are in runtime.cpp; the loop kernels in loop_engine.hpp.
// Part of runtime.cpp's translation unit (included at its end, before loop_engine.hpp, nowhere else), as the other *_engine.hpp are.
//
// A connected component of pending work that does not fit one launch (12 inputs / 8 outputs / 15 live values / 128
// micro-ops) is cut into consecutive SEGMENTS of its topological order.  Every prefix of a topological order is closed
// under dependencies, so a segment only reads materialised vectors and outputs of earlier segments; its outputs are the
// values somebody outside the segment still needs.  Each segment is the longest one that still fits (found once per
// component SHAPE and cached); components of identical shape — e.g. the same Euler step of several parameter sets — are
// cut identically and their segments run as rows of the same launches.
#include "runtime.hpp"

namespace fm {

// uses: per position of the component's order, the consumers INSIDE the component (structural: equal for all members of a group)
bool Engine::segment_dag(const BigDag& big, size_t s, size_t e, Dag& dag, const std::vector<int32_t>& uses) {
    const uint64_t ep = ++epoch_, ep_leaf = ++epoch_;          // mark == ep: produced inside the segment; == ep_leaf: registered input
    dag = Dag();
    for (size_t i = s; i < e; ++i) { Node* nd = big.order[i]; nd->mark = ep; nd->tmp_uses = 0; }
    for (size_t i = s; i < e; ++i) {
        Node* nd = big.order[i];
        for (int k = 0; k < nd->n_in; ++k) {
            Node* c = nd->in[k];
            if (c->mark == ep) { c->tmp_uses++; continue; }
            if (c->mark == ep_leaf) continue;
            if (!c->buf) return false;                          // reads a value that is neither materialised nor produced here: not a valid cut
            c->mark = ep_leaf;
            dag.leaves.push_back(c);
            if ((int)dag.leaves.size() > FM_MAX_IN) return false;
        }
    }
    if (e - s > (size_t)FM_MAX_OPS) return false;
    dag.order.assign(big.order.begin() + (std::ptrdiff_t)s, big.order.begin() + (std::ptrdiff_t)e);
    emit_ssa(dag);
    for (size_t i = s; i < e; ++i) {
        Node* nd = big.order[i];
        // an output of the component (build_big's decision — a handle alone does not make one), a consumer in a later segment, or the
        // component's root (also where its value has been given up: a segment cannot take the moments along, it stores it all the same)
        if (big.escapes[i] || uses[i] > nd->tmp_uses || (uses[i] == 0 && nd->refs_ext > 0)) { dag.outs.push_back(nd); dag.out_ids.push_back(nd->tmp_id); }
    }
    if (dag.outs.empty() || (int)dag.outs.size() > FM_MAX_OUT) return false;
    dag.roots = dag.outs;
    dag.sig.push_back((char)0xff);
    for (int v : dag.out_ids) dag.sig.push_back((char)(v + 1));
    return true;
}

// A value of a member without nodes has been computed: it is kept for the launches that read it, and handed to the copy's root node
// if it is one of the replicated roots.
void Engine::commit_described(BigDag& big, size_t pos, Buffer* b) {
    big.temp[pos] = b;                                  // owns the buffer's first reference
    const int32_t root = big.view->rep_root[pos];
    if (root < 0) return;
    const ReplicaGroup* g = big.view->g;
    Node* c = g->copy_roots[(size_t)big.copy * g->n_roots + root];
    b->refs++;
    commit_node(c, b);
}

// One segment of a planned component for every member of a group: gather the row blocks by index, launch, commit.
void Engine::run_planned_segment(const BigPlan::Seg& seg, std::vector<BigDag>& group, size_t first, size_t count, ReduceRequest* rr, Program* prog_red) {
    const int64_t n = group[first].n;
    const size_t n_scal = seg.scal.empty() ? 1 : seg.scal.size();
    std::vector<RowSpec> rows(count);
    std::vector<float> scalars(count * n_scal, 0.0f);
    std::vector<Stored> stored;
    stored.reserve(count * seg.out.size());
    try {
        for (size_t c = 0; c < count; ++c) {
            BigDag& big = group[first + c];
            RowSpec& r = rows[c];
            r.in.reserve(seg.in.size()); r.out.reserve(seg.out.size());
            for (int32_t i : seg.in) {
                Buffer* b = i >= 0 ? big.value((size_t)i) : big.leaves[(size_t)(-1 - i)]->buf;
                if (!b) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "planned segment reads a value that has not been computed");
                r.in.push_back(b->ptr);
            }
            for (size_t k = 0; k < seg.out.size(); ++k) { Buffer* b = new_buffer(n); stored.push_back({ &big, (size_t)seg.out[k], nullptr, b }); r.out.push_back(b->ptr); }
            float* sc = scalars.data() + c * n_scal;
            for (size_t k = 0; k < seg.scal.size(); ++k) sc[k] = big.scalar_at((size_t)seg.scal[k]);
            r.scalars = sc; r.shifts = rr ? &rr->shift : nullptr;
        }
        if (rr) { launch(prog_red, n, rows, rr->host_out, rr->dev_out); rr->done = true; }
        else launch(seg.prog, n, rows, nullptr, nullptr);
    } catch (...) { for (Stored& o : stored) buffer_unref(o.buf); throw; }
    commit_stored(stored);
}

// A kernel of the specialised tier on demand: asked for when its slot is empty — with FMHIP_JIT=sync also while it still waits for the
// worker: the caller compiles it now —; true when it is there.
template <class Source> bool Engine::kernel_ready(std::shared_ptr<JitSlot>& slot, Source&& source, int elems) {
    const bool sync = jit_mode == FMHIP_JIT_SYNC;
    if (!slot || (sync && slot->state.load(std::memory_order_acquire) == JitSlot::QUEUED)) {
        std::string text = source();
        if (text.empty()) return false;
        slot = jit().request_source(std::move(text), elems, sync);
    }
    return slot && slot->state.load(std::memory_order_acquire) == JitSlot::READY;
}

struct Engine::TempGuard {
    Engine* e; std::vector<BigDag>& g;
    static void drop(Engine* e, BigDag& b) { if (b.described()) for (Buffer*& t : b.temp) if (t) { e->buffer_unref(t); t = nullptr; } }
    ~TempGuard() { for (BigDag& b : g) drop(e, b); }
};

struct Engine::OperandTable {
    std::unordered_map<const Node*, int32_t> index_of;          // position in the order; a leaf: -1 - its number
    std::vector<std::array<int32_t, 3>> operand;                 // per operation
    explicit OperandTable(const BigDag& g) : operand(g.order.size()) {
        index_of.reserve(g.order.size() + g.leaves.size());
        for (size_t i = 0; i < g.order.size(); ++i) index_of[g.order[i]] = (int32_t)i;
        for (size_t i = 0; i < g.leaves.size(); ++i) index_of[g.leaves[i]] = -1 - (int32_t)i;
        for (size_t i = 0; i < g.order.size(); ++i)
            for (int k = 0; k < g.order[i]->n_in; ++k) operand[i][(size_t)k] = index_of.at(g.order[i]->in[k]);
    }
};

// The root of a component that has exactly one, as its LAST operation — its node (for a copy that exists as a description: the copy's
// root node) or nullptr.  g0 = the member that carries the order.
Node* Engine::single_root(const BigDag& b, const BigDag& g0)
{
    if (!b.described()) return (b.roots.size() == 1 && !b.order.empty() && b.order.back() == b.roots[0]) ? b.roots[0] : nullptr;
    const std::vector<int32_t>& rep_root = b.view->rep_root;
    const size_t n = g0.order.size();
    if (rep_root.size() != n || n == 0 || rep_root[n - 1] < 0) return nullptr;
    for (size_t i = 0; i + 1 < n; ++i) if (rep_root[i] >= 0) return nullptr;
    const ReplicaGroup* g = b.view->g;
    return g->copy_roots[(size_t)b.copy * g->n_roots + (size_t)rep_root[n - 1]];
}

// ---------------------------------------------------------------- a shape's plan over a group: run_plan and its steps

// The FMHIP_BATCH_TRACE lines of a plan (a flush that takes the moments of its roots along only)
void Engine::trace_batch(const BigPlan& plan, const std::vector<BigDag>& group, const ReduceRequest* rr, bool peeled) const {
    if (!batch_trace_on()) return;
    const BigDag& g0 = group[0];
    const BigPlan::Rolled::Peeled& pe = plan.rolled.peeled;
    if (!peeled)
        std::fprintf(stderr, "[fmhip batch] plan for a group of %zu, %zu nodes, %zu roots: rolled %d peeled %d segs %zu\n", group.size(), g0.order.size(), g0.roots.size(), plan.rolled.present ? 1 : 0, pe.present ? 1 : 0, plan.segs.size());
    else
        std::fprintf(stderr, "[fmhip batch] peeled group of %zu, %zu nodes: rr %d source_red %d roots %zu root_last %d\n", group.size(), g0.order.size(), rr ? 1 : 0, pe.source_red.empty() ? 0 : 1, g0.roots.size(), (int)(!g0.order.empty() && !g0.roots.empty() && g0.order.back() == g0.roots[0]));
}

static size_t peeled_tiles(const std::shared_ptr<JitSlot>& jit, int64_t n) { return (size_t)((n + (int64_t)FM_BLOCK * jit->elems - 1) / ((int64_t)FM_BLOCK * jit->elems)); }

// The peeled form — head, loop and tail of the component in one launch.  A caller that values one product after the other (1 row x
// 489 tiles) turns three launches of ≈ 9 + 20 + 8 µs into one; the lock-step batches of the native driver save the stores and loads
// of the values between the parts (measured on the 1 M-path calibration, same box: 12 671 → 4 639 launches, 2.65 → 2.50 s of
// kernel time with the head and the tail limited to 128 operations each).  Its gate: the shape has one, the JIT tier is on, the kernel
// is there (asked for here), there is something to compute, FMHIP_PEEL_MAX_WORKGROUPS (it limits the form to small launches), and the
// row table of the whole group — ONE launch, however many members — fits the pinned ring.
bool Engine::peeled_applies(BigPlan& plan, const std::vector<BigDag>& group) {
    BigPlan::Rolled::Peeled& pe = plan.rolled.peeled;
    if (!(pe.present && jit_mode != FMHIP_JIT_OFF && kernel_ready(pe.jit, [&] { return pe.source; }, pe.elems) && group[0].n > 0)) return false;
    static const size_t PEEL_MAX_WORKGROUPS = knob_size("FMHIP_PEEL_MAX_WORKGROUPS", ~(size_t)0);
    return group.size() * peeled_tiles(pe.jit, group[0].n) <= PEEL_MAX_WORKGROUPS && ring_rows(pe.row_words) >= group.size();
}

// The peeled launch of the whole group, with the moments it can take along; false: it did not run, the segments do.  Whose moments:
// the caller's request (`chain.getAverage()` on the root of a single component: a workgroup's tile is one unit of the reduction tree — a
// product of a caller that values one after the other is ONE launch, and its value is not read again); or, in a flush that collects the
// moments of all pending roots (Engine::reduce), those of every member, as rows of this launch; or none.  A plan whose root is wanted
// for its moments only has peeled kernels that do not store it: usable only when this launch takes the moments of every member's root;
// otherwise the segments run (they go by the nodes' references and store it).
bool Engine::run_peeled_group(BigPlan& plan, std::vector<BigDag>& group, ReduceRequest* rr) {
    BigPlan::Rolled::Peeled& pe = plan.rolled.peeled;
    TempGuard guard{ this, group };
    const bool can_reduce = !pe.source_red.empty() && peeled_tiles(pe.jit, group[0].n) <= (size_t)FM_SPAN_UNITS * 65536;
    auto red_ready = [&] { return kernel_ready(pe.jit_red, [&] { return pe.source_red; }, pe.elems); };
    ReduceRequest* fused = nullptr;
    if (rr && group.size() == 1 && !group[0].described() && can_reduce && group[0].order.back() == group[0].roots[0] && red_ready()) fused = rr;
    trace_batch(plan, group, rr, true);
    ReduceRequest every{ 0.0, nullptr, nullptr, false };
    RootMoments along;
    std::vector<Node*> root_nodes;
    if (!fused && want_root_moments_ && !rr && can_reduce) {
        bool roots_only = true;
        for (const BigDag& b : group) { Node* r = single_root(b, group[0]); root_nodes.push_back(r); roots_only &= r != nullptr && !r->moments_blocked && (!plan.discards_root || r->discard); }
        if (roots_only && red_ready() && along.open(*this, group.size())) { every.host_out = along.host(); every.dev_out = along.dev(); fused = &every; }
    }
    if (plan.discards_root && fused != &every) return false;
    std::vector<uint32_t> row_of;
    run_peeled(plan.rolled, group, 0, group.size(), fused, &row_of);
    if (fused != &every || !every.done) return true;
    for (size_t i = 0; i < root_nodes.size(); ++i) along.deliver(root_nodes[i], every.dev_out ? (size_t)row_of[i] : i);       // (arena slots are per row: members of a common row, the same slot)
    if (plan.discards_root)                         // moments taken, value not stored: not a root of later flushes; what it was computed from is let go
        for (Node* r : root_nodes) if (!r->buf) give_up_value(r);
    return true;
}

// This shape has never run as segments: its members with nodes take the general path now (plan_segments), which leaves the cuts in the
// plan; the copies that exist as a description run from them.
void Engine::cut_on_first_use(BigPlan& plan, std::vector<BigDag>& group) {
    std::vector<BigDag> described, with_nodes;
    for (BigDag& b : group) (b.described() ? described : with_nodes).push_back(std::move(b));
    if (with_nodes.empty()) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "a group of copies without their original");
    plan_segments(plan, with_nodes);
    if (!described.empty()) run_plan(plan, described);
}

// The variant of the last segment that also reduces the component's root, for `chain.getAverage()` on a single large expression: one
// launch and one read of the root less than a stand-alone reduction behind the segment.  Only when that variant accumulates like
// the stand-alone reduction program does (8 elements per lane: the sums are then the same to the last bit).  nullptr: there is none.
Program* Engine::last_segment_reducer(BigPlan& plan, const std::vector<BigDag>& group, bool rolled, const ReduceRequest* rr) {
    if (!rr || group.size() != 1 || group[0].described() || plan.segs.empty()) return nullptr;
    BigPlan::Seg& last = plan.segs.back();
    const BigDag& g0 = group[0];
    const int32_t root_pos = (int32_t)g0.order.size() - 1;
    size_t k_root = last.out.size();
    for (size_t k = 0; k < last.out.size(); ++k) if (last.out[k] == root_pos) k_root = k;
    // (the size gate of reduce(): a launch with a fused reduction has one workgroup per 8192 elements of a row — fine for a segment
    // over two input vectors, a starved launch for one over eleven)
    if ((rolled && last.zone == 1) || last.no_red || last.ssa.empty() || k_root == last.out.size() || g0.order[(size_t)root_pos] != g0.roots[0] ||
        !(g0.n * (int64_t)last.n_in <= (int64_t(1) << 21) || unit_launch(g0.n, 1))) return nullptr;
    if (!last.prog_red) {
        try { last.prog_red = compile(last.ssa, last.n_in, last.out_ids, { last.out_ids[k_root] }, nullptr, false); }
        catch (const Error& e) { if (e.code != FMHIP_ERR_PROGRAM_LIMIT) throw; last.no_red = true; }
        if (last.prog_red && last.prog_red->proto.variant != 1u) { delete last.prog_red; last.prog_red = nullptr; last.no_red = true; }
    }
    return last.prog_red;
}

// Segment by segment, MAX_LAUNCH_ROWS members per launch; the loop's stretch as launches of the rolled kernel (rolled_batch members
// each; 0: as its segments); the last segment through prog_red where there is one.  Members without nodes give the values no later
// segment reads back to the pool as they go.
void Engine::run_segments(BigPlan& plan, std::vector<BigDag>& group, size_t rolled_batch, ReduceRequest* rr, Program* prog_red) {
    bool any_described = false;
    for (const BigDag& b : group) any_described |= b.described();
    auto release_temps = [&](const std::vector<int32_t>& positions) {
        if (!any_described) return;
        for (BigDag& b : group) {
            if (!b.described()) continue;
            for (int32_t pos : positions) if (Buffer* t = b.temp[(size_t)pos]) { b.temp[(size_t)pos] = nullptr; buffer_unref(t); }
        }
    };
    bool rolled_done = false;
    for (size_t si = 0; si < plan.segs.size(); ++si) {
        const BigPlan::Seg& seg = plan.segs[si];
        if (rolled_batch && seg.zone == 1) {        // the loop's stretch: one launch of the rolled kernel instead of its segments
            if (!rolled_done) for (size_t off = 0; off < group.size(); off += rolled_batch) run_rolled(plan.rolled, group, off, std::min(rolled_batch, group.size() - off));
            rolled_done = true;
        } else if (prog_red && si + 1 == plan.segs.size())
            run_planned_segment(seg, group, 0, 1, rr, prog_red);
        else
            for (size_t off = 0; off < group.size(); off += MAX_LAUNCH_ROWS) run_planned_segment(seg, group, off, std::min(MAX_LAUNCH_ROWS, group.size() - off));
        release_temps(seg.free_after);
    }
}

// A component shape with a plan, for every member of a group.  The rolled launch carries one row table for all its members through the
// pinned ring (≈ 5 KB per row for the LMM step, but iterations x (inputs + outputs) words in general): as many members per launch as
// fit; a single row that does not fit, or a kernel that is not there (it is asked for here), leaves the stretch to its segments.
void Engine::run_plan(BigPlan& plan, std::vector<BigDag>& group, ReduceRequest* rr) {
    trace_batch(plan, group, rr, false);
    const bool rolled = plan.rolled.present && jit_mode != FMHIP_JIT_OFF && kernel_ready(plan.rolled.jit, [&] { return plan.rolled.source; }, plan.rolled.elems);
    const size_t rolled_batch = rolled ? rows_per_launch(plan.rolled.row_words) : 0;
    if (peeled_applies(plan, group) && run_peeled_group(plan, group, rr)) return;
    if (plan.segs_missing) { cut_on_first_use(plan, group); return; }
    TempGuard guard{ this, group };
    run_segments(plan, group, rolled_batch, rr, last_segment_reducer(plan, group, rolled_batch > 0, rr));
}

// ---------------------------------------------------------------- the general path: a shape is cut (plan_segments and its steps)

// (a) The end of the longest segment starting at s, not beyond `limit`, that fits one launch and compiles.  Inputs grow monotonically with
// the end; outputs and live values do not: every end that passes the cheap checks is collected, the largest one that also compiles is
// taken (its program stays in program_cache_).
size_t Engine::longest_segment(const BigDag& g0, size_t s, size_t limit, const std::vector<int32_t>& uses) {
    std::vector<size_t> cheap;
    for (size_t cand = s + 1; cand <= limit && cand - s <= (size_t)FM_MAX_OPS; ++cand) {
        Dag d;
        if (segment_dag(g0, s, cand, d, uses)) cheap.push_back(cand);
        else if ((int)d.leaves.size() > FM_MAX_IN) break;
    }
    for (size_t k = cheap.size(); k-- > 0;) {
        Dag d;
        segment_dag(g0, s, cheap[k], d, uses);
        if (!program_cache_.count(d.sig)) {
            try { program_cache_[d.sig] = compile(d.ops, (int)d.leaves.size(), d.out_ids, {}, nullptr, false); }
            catch (const Error& err) { if (err.code == FMHIP_ERR_PROGRAM_LIMIT) continue; throw; }
        }
        return cheap[k];
    }
    throw Error(FMHIP_ERR_PROGRAM_LIMIT, "an operation does not fit one launch");
}

// (b) The segment [s, e) of g0, whose Dag is d, as the plan keeps it: its program, where its row block comes from (positions of g0's
// order; leaves: -1 - number), and, of the component's LAST segment, what the variant that reduces the root is compiled from.
Engine::BigPlan::Seg Engine::describe_segment(const Dag& d, const BigDag& g0, const OperandTable& table, size_t s, size_t e, int zone) {
    BigPlan::Seg seg;
    seg.prog = program_cache_.at(d.sig);
    for (Node* l : d.leaves) seg.in.push_back(table.index_of.at(l));
    for (Node* o : d.outs) seg.out.push_back(table.index_of.at(o));
    for (size_t i = s; i < e; ++i) if (op_info(g0.order[i]->opcode).scalar) seg.scal.push_back((int32_t)i);
    seg.zone = zone;
    if (e == g0.order.size()) { seg.ssa = d.ops; seg.out_ids = d.out_ids; seg.n_in = (int)d.leaves.size(); }
    return seg;
}

// (c) The Dags of one segment, one per member, run as rows of the same launches (they are consumed).
void Engine::run_cut_segment(std::vector<Dag>& dags) {
    for (size_t off = 0; off < dags.size(); off += MAX_LAUNCH_ROWS) {
        std::vector<Dag> part(std::make_move_iterator(dags.begin() + off), std::make_move_iterator(dags.begin() + std::min(dags.size(), off + MAX_LAUNCH_ROWS)));
        if (!run_dags(part)) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "segment of a split component does not fit one launch");
    }
}

// The cuts are COMMITTED WHOLE: the plan receives them when the last segment has run, here, where nothing can throw between the first
// word written and the last — the values no later segment reads (members without nodes give them back to the pool there) are worked out
// on the local list first; then the plan takes the list, its reference on every program (pool_purge drops both caches together), and no
// longer misses its segments.  A cutting that fails leaves the plan as it was: the shape is cut afresh when it comes round again.
void Engine::commit_cuts(BigPlan& plan, std::vector<BigPlan::Seg>& cuts) {
    std::unordered_map<int32_t, size_t> last_reader;
    for (size_t k = 0; k < cuts.size(); ++k) for (int32_t i : cuts[k].in) if (i >= 0) last_reader[i] = k;
    for (const auto& kv : last_reader) cuts[kv.second].free_after.push_back(kv.first);       // (still the local list; from here on nothing throws)
    plan.segs.swap(cuts);
    for (BigPlan::Seg& seg : plan.segs) seg.prog->refs++;
    plan.segs_missing = false;
}

// The general path: the members WITH nodes of a group whose shape has no segments yet are cut into launches (longest segment that fits
// one launch, again and again; cuts forced at the ends of the loop plan.rolled describes, so that either form can run between them) and
// run segment by segment; the cuts reach the plan when the last one has run (commit_cuts).
void Engine::plan_segments(BigPlan& plan, std::vector<BigDag>& group) {
    const BigDag& g0 = group[0];
    const size_t n_ops = g0.order.size();
    const OperandTable table(g0);                           // node -> index in group[0] for the plan (segment_dag reuses the nodes' scratch fields)
    std::vector<int32_t> uses(n_ops, 0);                    // consumers inside the component, per position (before anything runs)
    for (size_t i = 0; i < n_ops; ++i)
        for (int k = 0; k < g0.order[i]->n_in; ++k) { const int32_t o = table.operand[i][(size_t)k]; if (o >= 0) uses[(size_t)o]++; }
    size_t zone_begin = n_ops, zone_end = n_ops;
    if (plan.rolled.present) { zone_begin = plan.rolled.begin; zone_end = zone_begin + (size_t)plan.rolled.period * plan.rolled.iterations; }
    std::vector<BigPlan::Seg> cuts;
    for (size_t s = 0, e = 0; s < n_ops; s = e) {
        const int zone = s < zone_begin ? 0 : (s < zone_end ? 1 : 2);                          // a segment never crosses an end of the loop
        e = longest_segment(g0, s, zone == 0 ? zone_begin : (zone == 1 ? zone_end : n_ops), uses);
        std::vector<Dag> dags(group.size());
        for (size_t c = 0; c < group.size(); ++c)
            if (!segment_dag(group[c], s, e, dags[c], uses)) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "inconsistent segment of a split component");
        cuts.push_back(describe_segment(dags[0], g0, table, s, e, zone));
        run_cut_segment(dags);
    }
    commit_cuts(plan, cuts);
}

// ---------------------------------------------------------------- the entry: a group of components of one shape

void Engine::run_big_group(std::vector<BigDag>& group, ReduceRequest* rr) {
    HostTimer timer(HostProfile::RUN_BIG);
    BigDag& g0 = group[0];
    auto planned = plan_cache_.find(g0.hash);
    if (planned != plan_cache_.end() && planned->second.sig != g0.sig) planned = plan_cache_.end();       // hash collision: general path, nothing cached
    const bool collision = planned == plan_cache_.end() && plan_cache_.count(g0.hash) != 0;
    if (planned != plan_cache_.end()) { run_plan(planned->second, group, rr); return; }
    // First component of this shape.  Its loop, if it has one, is found first: a periodic stretch of the order becomes a rolled loop (one
    // launch) as soon as its kernel exists; segments remain its fallback.
    BigPlan plan;
    size_t first_with_nodes = 0;
    while (first_with_nodes < group.size() && group[first_with_nodes].described()) ++first_with_nodes;
    if (first_with_nodes == group.size()) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "a group of copies without their original");
    plan_loop(plan, group[first_with_nodes]);
    plan.sig = g0.sig;
    plan.discards_root = g0.discard_root;
    plan.segs_missing = true;
    if (collision) {                                        // (practically never) nothing is cached: the plan lives for this group only, and gives its programs back
        struct Uncached { BigPlan& p; ~Uncached() { for (BigPlan::Seg& seg : p.segs) seg.prog->refs--; } } uncached{ plan };
        cut_on_first_use(plan, group);
        return;
    }
    // The plan is written down WITHOUT its segments: where the whole component is one launch of a kernel that exists already (the peeled
    // form, from the code-object caches or the build-time pack) nothing else is ever needed; run_plan cuts the segments — by running the
    // component through the general path — the first time that launch is not available (until round 5 every shape's first occurrence ran as
    // segments on the interpreter, whatever kernels existed: a tenth of a second per calibration, and again for every variant of a shape
    // the escape policy moves through).
    BigPlan& cached = plan_cache_[g0.hash];
    cached = std::move(plan);
    run_plan(cached, group, rr);
}

} // namespace fm
