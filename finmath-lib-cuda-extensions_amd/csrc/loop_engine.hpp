// loop_engine.hpp — the rolled and peeled loop kernels' host side: finding the periodic stretch of a large component (detect_loop), its
// peeled form (plan_peel), asking for their kernels (plan_loop) and running them over a group (run_rolled, run_peeled); and what every
// launch of a loop kernel shares, the merged ones of merged_chains_engine.hpp included: one row-table launch (launch_row_table), the rows
// that are computed once (CommonRows) and who else receives what they store (share_common_rows).  Part of runtime.cpp's translation unit
// (included at its end, nowhere else): Engine member functions in a file of their own because runtime.cpp is long enough, and in that
// translation unit so that every build that lists the engine's sources — the library's, the sanitizer builds against the null device —
// has them without being told.  run_plan, plan_segments and run_big_group, which decide WHEN a loop kernel runs, are in plans_engine.hpp.
//
// The scheduled order of a large component is often PERIODIC: the same few operations over one vector after another, each
// iteration feeding the next through a value or two — the running factor sum over the LIBOR components of an Euler step, a
// swap's backward induction over its periods.  Cut into launches of ≤ 12 inputs / 8 outputs such a stretch moves ≈ 1.5 vectors
// per iteration and step and costs a launch every six iterations.  Rolled up it is ONE launch: the body of one iteration is
// compiled (hiprtc) into a kernel that loops over the iterations, keeps the carried values in registers, loads each iteration's
// inputs while it computes the previous one and stores each result the moment it is final; iteration count, vector pointers and
// scalar operands come from the row table, so one kernel serves every component count.  Every operation is evaluated by the
// same ueval<> functions in the same order per element as in the segmented launches: results are bit-identical, and until the
// kernel is compiled (or with FMHIP_JIT=off / FMHIP_ROLL=0) the segmented launches run.
#include "runtime.hpp"

namespace fm {

static inline uint64_t mix64(uint64_t h, uint64_t v) { h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2); return h * 0xff51afd7ed558ccdull; }

// an operation of a loop kernel's text: the micro-op of the node's opcode over its operands by name (false: the opcode has none)
static bool loop_op(const Node* nd, int math_mode, const std::string* name, RolledBody::Op& out) {
    UVariant uv{};
    if (!micro_op_for(nd->opcode, 0, math_mode, &uv)) return false;
    out = { uv.uop, name[0], uv.r1_pos >= 0 ? name[uv.r1_pos] : std::string(), uv.r2_pos >= 0 ? name[uv.r2_pos] : std::string(), op_info(nd->opcode).scalar };
    return true;
}

#define ROLL_TRACE(...) do { if (roll_trace) std::fprintf(stderr, __VA_ARGS__); } while (0)
bool Engine::detect_loop(const BigDag& g, const std::vector<std::array<int32_t, 3>>& operand, BigPlan::Rolled& ro, std::string* source, int* elems_out, RolledBody* body_out)
{
    static const bool roll_trace = std::getenv("FMHIP_ROLL_TRACE") != nullptr;
    const size_t n = g.order.size();
    ROLL_TRACE("[fmhip roll] component of %zu nodes, %zu leaves\n", n, g.leaves.size());
    const int MAX_PERIOD = 128, MIN_ITERATIONS = 5, GLOBAL_SPAN = MAX_PERIOD;      // an input of ONE iteration has all its uses less than a period apart
    if (n < 48) return false;
    std::vector<int32_t> first_use(g.leaves.size(), -1), last_leaf_use(g.leaves.size(), -1);
    std::vector<uint32_t> last_use(n, 0);                       // largest consumer index; n = needed outside the component
    for (size_t i = 0; i < n; ++i) {
        if (g.escapes[i]) last_use[i] = (uint32_t)n;
        for (int k = 0; k < g.order[i]->n_in; ++k) {
            const int32_t o = operand[i][(size_t)k];
            if (o < 0) { const size_t l = (size_t)(-1 - o); if (first_use[l] < 0) first_use[l] = (int32_t)i; last_leaf_use[l] = (int32_t)i; }
            else if (last_use[(size_t)o] < (uint32_t)i) last_use[(size_t)o] = (uint32_t)i;
        }
    }
    auto is_global = [&](size_t l) { return last_leaf_use[l] - first_use[l] >= GLOBAL_SPAN; };
    // position-independent signature of every node: what it does and how far back its operands are.  NOT whether it is stored: an
    // iteration that stores a value the others only pass on (a state one product reads, a handle the escape policy keeps for one
    // component and not for the next) is the same iteration — the loop stores that position in EVERY iteration (out_needed below is the
    // union over the iterations): a few vectors more written, against a stretch that would not roll at all.
    std::vector<uint64_t> sig(n);
    for (size_t i = 0; i < n; ++i) {
        const Node* nd = g.order[i];
        uint64_t h = mix64(0x1234, (uint64_t)nd->opcode * 8 + (uint64_t)nd->n_in * 2);
        for (int k = 0; k < nd->n_in; ++k) {
            const int32_t o = operand[i][(size_t)k];
            if (o >= 0) h = mix64(h, 0x100000000ull + (uint64_t)((int64_t)i - o));
            else { const size_t l = (size_t)(-1 - o); h = is_global(l) ? mix64(h, 0x200000000ull + l) : mix64(h, 0x300000000ull + (uint64_t)((int64_t)i - first_use[l])); }
        }
        sig[i] = h;
    }
    // the periodic stretch that covers the most nodes
    size_t best_start = 0, best_cover = 0; int best_period = 0;
    for (int P = 3; P <= MAX_PERIOD && (size_t)P * MIN_ITERATIONS <= n; ++P) {
        size_t run_start = 0, run = 0;
        for (size_t i = 0; i + (size_t)P <= n; ++i) {
            const bool match = i + (size_t)P < n && sig[i] == sig[i + (size_t)P];
            if (match) { if (run == 0) run_start = i; ++run; }
            if (!match || i + (size_t)P + 1 >= n) {
                if (run > 0) { const size_t cover = (run + (size_t)P) / (size_t)P * (size_t)P; if (cover > best_cover) { best_cover = cover; best_start = run_start; best_period = P; } }
                run = 0;
            }
        }
    }
    ROLL_TRACE("[fmhip roll]   best period %d, start %zu, cover %zu\n", best_period, best_start, best_cover);
    if (best_period == 0 || best_cover / (size_t)best_period < (size_t)MIN_ITERATIONS) return false;
    const uint32_t P = (uint32_t)best_period;
    // phase: any rotation of the period is periodic too; take the one with the fewest values crossing the iteration boundary
    uint32_t best_phase = 0; size_t best_carried = SIZE_MAX;
    for (uint32_t phase = 0; phase < P; ++phase) {
        const size_t b = best_start + P + phase;                // second detected iteration: its predecessors exist
        if (b + P > best_start + best_cover) break;
        std::unordered_set<int32_t> crossing;
        bool ok = true;
        for (uint32_t q = 0; q < P && ok; ++q)
            for (int k = 0; k < g.order[b + q]->n_in; ++k) {
                const int32_t o = operand[b + q][(size_t)k];
                if (o < 0) {                                    // an input of one iteration must not straddle the boundary either
                    const size_t l = (size_t)(-1 - o);
                    if (!is_global(l) && ((size_t)first_use[l] < b || (size_t)last_leaf_use[l] >= b + P)) { ok = false; break; }
                    continue;
                }
                const int64_t d = (int64_t)(b + q) - o;
                if (d > (int64_t)q) { if (d > (int64_t)q + P) { ok = false; break; } crossing.insert(o); }
            }
        if (ok && crossing.size() < best_carried) { best_carried = crossing.size(); best_phase = phase; }
    }
    ROLL_TRACE("[fmhip roll]   phase %u, %zu values cross the iteration boundary\n", best_phase, best_carried == SIZE_MAX ? (size_t)0 : best_carried);
    if (best_carried == SIZE_MAX) return false;
    const size_t begin = best_start + P + best_phase;
    const size_t R = (best_start + best_cover - begin) / P;
    if (R < (size_t)MIN_ITERATIONS - 1) return false;
    const size_t end = begin + R * P;
    // validate every iteration; collect the body's interface from the first one
    std::vector<char> out_needed(P, 0), final_needed(P, 0);
    for (size_t r = 0; r < R; ++r)
        for (uint32_t q = 0; q < P; ++q) {
            const size_t i = begin + r * P + q;
            if (sig[i] != sig[begin + q]) { ROLL_TRACE("[fmhip roll]   aperiodic at iteration %zu position %u\n", r, q); return false; }
            for (int k = 0; k < g.order[i]->n_in; ++k) {
                const int32_t o = operand[i][(size_t)k];
                if (o >= 0) { const int64_t d = (int64_t)i - o; if (d > (int64_t)q + P) { ROLL_TRACE("[fmhip roll]   operand further back than one iteration (iteration %zu position %u)\n", r, q); return false; } }
                else {
                    const size_t l = (size_t)(-1 - o);
                    if (!is_global(l) && ((size_t)first_use[l] < begin + r * P || (size_t)last_leaf_use[l] >= begin + (r + 1) * P)) {   // an input of exactly one iteration
                        ROLL_TRACE("[fmhip roll]   input used by more than one iteration (iteration %zu position %u, span %d)\n", r, q, last_leaf_use[l] - first_use[l]); return false; }
                }
            }
            // consumers in the same and in the next iteration are served from registers; anybody later (or outside) needs the vector
            const size_t reach = r + 1 < R ? begin + (r + 2) * P : end;
            if (last_use[i] >= reach) { if (r + 1 == R && !g.escapes[i]) final_needed[q] = 1; else out_needed[q] = 1; }     // last iteration only: stored once, behind the loop
        }
    ro = BigPlan::Rolled();
    ro.begin = (uint32_t)begin; ro.period = P; ro.iterations = (uint32_t)R;
    std::vector<int> carried_index(P, -1), global_index(g.leaves.size(), -1);
    std::vector<std::array<std::string, 3>> name(P);              // operand names of the body
    bool library_math = false, uses_log = false;
    int n_local_leaf = 0;
    std::unordered_map<size_t, int> local_leaf;                      // leaf -> per-iteration input number (first iteration's leaves)
    for (uint32_t q = 0; q < P; ++q) {
        const size_t i = begin + q;
        const Node* nd = g.order[i];
        library_math |= nd->opcode == FMHIP_OP_POW_S || nd->opcode == FMHIP_OP_SIN || nd->opcode == FMHIP_OP_COS || nd->opcode == FMHIP_OP_EXP || nd->opcode == FMHIP_OP_LOG;
        uses_log |= nd->opcode == FMHIP_OP_LOG && math_mode != FMHIP_MATH_FAST;
        if (op_info(nd->opcode).scalar) ro.scal_pos.push_back(q);
        if (out_needed[q]) ro.out_pos.push_back(q);
        else if (final_needed[q]) ro.final_pos.push_back(q);
        for (int k = 0; k < nd->n_in; ++k) {
            const int32_t o = operand[i][(size_t)k];
            if (o >= 0) {
                const int64_t d = (int64_t)i - o;
                if (d <= (int64_t)q) name[q][(size_t)k] = "v" + std::to_string(q - (uint32_t)d);
                else {
                    const uint32_t src = q + P - (uint32_t)d;
                    if (carried_index[src] < 0) { carried_index[src] = (int)ro.carried.size(); ro.carried.push_back(src); }
                    name[q][(size_t)k] = "c" + std::to_string(carried_index[src]);
                }
            } else {
                const size_t l = (size_t)(-1 - o);
                if (is_global(l)) {
                    if (global_index[l] < 0) { global_index[l] = (int)ro.global_leaf.size(); ro.global_leaf.push_back((int32_t)l); }
                    name[q][(size_t)k] = "g" + std::to_string(global_index[l]);
                } else {
                    auto it = local_leaf.find(l);
                    if (it == local_leaf.end()) { it = local_leaf.emplace(l, n_local_leaf++).first; ro.leaf_in.push_back({ q, (uint32_t)k }); }
                    name[q][(size_t)k] = "l" + std::to_string(it->second);
                }
            }
        }
    }
    const size_t G = ro.global_leaf.size(), CI = ro.carried.size(), CO = ro.final_pos.size(), LI = ro.leaf_in.size(), LO = ro.out_pos.size(), LS = ro.scal_pos.size();
    ROLL_TRACE("[fmhip roll]   begin %zu, %zu iterations of %u: %zu global, %zu carried, %zu in, %zu out, %zu scalars\n", begin, R, P, G, CI, LI, LO, LS);
    if (G > 8 || CI > 12 || CO > 12 || LI > 12 || LO > 12 || LO + CO == 0 || LS > 48) return false;
    ro.row_words = (uint32_t)(G + CI + CO + R * (LI + LO) + (R * LS + 1) / 2);
    ro.iter_leaf.resize(R * LI);
    for (size_t r = 0; r < R; ++r)
        for (size_t m2 = 0; m2 < LI; ++m2) ro.iter_leaf[r * LI + m2] = -1 - operand[begin + r * P + ro.leaf_in[m2].first][(size_t)ro.leaf_in[m2].second];
    // ---- the kernel
    // elements per lane: 8 keeps more bytes in flight per wave, 4 halves the registers (more waves per SIMD to overlap the loop's
    // load → compute → store with each other) — which loops with library mathematics need
    const int E = library_math ? 4 : 8;
    *elems_out = E;
    RolledBody body;
    body.elems = E; body.uses_log = uses_log; body.globals = (uint32_t)G; body.inputs = (uint32_t)LI;
    body.carried = ro.carried; body.final_pos = ro.final_pos; body.out_pos = ro.out_pos;
    for (uint32_t q = 0; q < P; ++q) {
        RolledBody::Op op;
        if (!loop_op(g.order[begin + q], math_mode, name[q].data(), op)) return false;
        body.ops.push_back(std::move(op));
    }
    jit().record(jit_describe(body));
    *source = jit_generate_rolled_source(body);
    if (body_out) *body_out = body;
    return true;
}

// The PEELED form of a component with a rolled loop: everything in front of the loop and behind it in the same launch (jit.hpp:
// RolledBody::Peel).  Possible when both parts are short, read few vectors of their own, and the part behind the loop reads nothing
// of the loop but final values of its last iteration.
bool Engine::plan_peel(const BigDag& g, const std::vector<std::array<int32_t, 3>>& operand, BigPlan::Rolled& ro, const RolledBody& loop_body)
{
    static const bool PEEL = knob_on("FMHIP_PEEL");
    if (!PEEL) return false;
    const size_t n = g.order.size(), P = ro.period, R = ro.iterations, begin = ro.begin, end = begin + P * R;
    static const size_t MAX_OPS = knob_size("FMHIP_PEEL_MAX_OPS", (size_t)192);
    const size_t MAX_EXTRA = 16;
    if (begin > MAX_OPS || n - end > MAX_OPS || begin == 0) return false;
    RolledBody body = loop_body;
    RolledBody::Peel& pl = body.peel;
    BigPlan::Rolled::Peeled pe;
    pl.present = true;
    std::vector<int> global_of(g.leaves.size(), -1), extra_of(g.leaves.size(), -1);
    for (size_t k = 0; k < ro.global_leaf.size(); ++k) global_of[(size_t)ro.global_leaf[k]] = (int)k;
    auto leaf_name = [&](size_t l) {
        if (global_of[l] >= 0) return "g" + std::to_string(global_of[l]);
        if (extra_of[l] < 0) { extra_of[l] = (int)pe.extra_leaf.size(); pe.extra_leaf.push_back((int32_t)l); }
        return "x" + std::to_string(extra_of[l]);
    };
    std::vector<int> final_of(P, -1);
    for (size_t k = 0; k < ro.final_pos.size(); ++k) final_of[ro.final_pos[k]] = (int)k;
    auto make_op = [&](size_t i, bool behind, RolledBody::Op& out) {
        const Node* nd = g.order[i];
        if (nd->opcode == FMHIP_OP_POW_S || nd->opcode == FMHIP_OP_SIN || nd->opcode == FMHIP_OP_COS) return false;     // out-of-line library code: not in these kernels
        std::string name[3];
        for (int k = 0; k < nd->n_in; ++k) {
            const int32_t o = operand[i][(size_t)k];
            if (o < 0) name[k] = leaf_name((size_t)(-1 - o));
            else if ((size_t)o < begin) name[k] = "p" + std::to_string(o);
            else if ((size_t)o >= end) { if (!behind) return false; name[k] = "q" + std::to_string((size_t)o - end); }
            else {                                                   // a value of the loop: only a final value of its LAST iteration, only from behind it
                const size_t it = ((size_t)o - begin) / P, q = ((size_t)o - begin) % P;
                if (!behind || it != R - 1 || final_of[q] < 0) return false;
                name[k] = "F" + std::to_string(final_of[q]);
            }
        }
        if (!loop_op(nd, math_mode, name, out)) return false;
        body.uses_log |= out.uop == U_LOG;
        return true;
    };
    for (size_t i = 0; i < begin; ++i) {
        RolledBody::Op op;
        if (!make_op(i, false, op)) return false;
        pl.pre.push_back(op);
        if (op.scalar) pe.pre_scal.push_back((uint32_t)i);
        if (g.escapes[i]) { pl.pre_out.push_back((uint32_t)i); pe.pre_out.push_back((uint32_t)i); }
    }
    pl.extra_pre = (uint32_t)pe.extra_leaf.size();
    for (size_t k = 0; k < ro.carried.size(); ++k) pl.carried_init.push_back("p" + std::to_string(begin - P + ro.carried[k]));
    for (size_t i = end; i < n; ++i) {
        RolledBody::Op op;
        if (!make_op(i, true, op)) return false;
        pl.post.push_back(op);
        if (op.scalar) pe.post_scal.push_back((uint32_t)i);
        if (g.escapes[i]) { pl.post_out.push_back((uint32_t)(i - end)); pe.post_out.push_back((uint32_t)i); }
    }
    pl.extra_post = (uint32_t)pe.extra_leaf.size() - pl.extra_pre;
    if (pe.extra_leaf.size() > MAX_EXTRA) return false;
    // a value of the loop that a later launch used to read (stored every iteration) must not be one the tail needed from an earlier
    // iteration: make_op has rejected those.  Final values are stored only where somebody outside the component reads them.
    for (size_t k = 0; k < ro.final_pos.size(); ++k) { const bool esc = g.escapes[begin + (R - 1) * P + ro.final_pos[k]] != 0; pl.final_store.push_back(esc ? 1u : 0u); pe.final_store.push_back(esc ? 1 : 0); }
    pe.n_pre_scal = (uint32_t)pe.pre_scal.size(); pe.n_post_scal = (uint32_t)pe.post_scal.size(); pe.n_ops = (uint32_t)n;
    const size_t NX = pe.extra_leaf.size(), G = ro.global_leaf.size(), CO = ro.final_pos.size(), NXO = pe.pre_out.size() + pe.post_out.size(), LI = ro.leaf_in.size(), LO = ro.out_pos.size(), LS = ro.scal_pos.size();
    pe.row_words = (uint32_t)(NX + G + CO + NXO + R * (LI + LO) + (pe.n_pre_scal + R * LS + pe.n_post_scal + 1) / 2);
    jit().record(jit_describe(body));
    pe.source = jit_generate_rolled_source(body);
    pe.elems = body.elems;
    pe.present = true;
    // the variant that also takes the moments of the component's root (its last operation), for `chain.getAverage()`
    if (body.elems == 8) {
        if (n > end) pl.reduce = "q" + std::to_string(n - 1 - end);
        else if (final_of[(n - 1 - begin) % P] >= 0) pl.reduce = "F" + std::to_string(final_of[(n - 1 - begin) % P]);
        if (!pl.reduce.empty()) { pe.desc_red = jit_describe(body); jit().record(pe.desc_red); pe.source_red = jit_generate_rolled_source(body);
                                  if (MERGE_CHAINS) pe.mergeable = merge_shape_index(pe.desc_red) >= 0 ? 1 : 0; }
    }
    ro.peeled = std::move(pe);
    return true;
}

// ---------------------------------------------------------------- what the launches of the loop kernels share

// One launch of a loop kernel over a table of `rows` rows: the kernel and its grid, the fused reduction it may carry, and what it adds to
// the engine's counters — the formulas differ per form (rolled, peeled, merged), so the figures come from the call site.
struct Engine::RowLaunch {
    const JitSlot* slot; const char* what;                      // what: "rolled" / "peeled" / "merged", in what an error says
    int64_t n, tiles; size_t rows, row_words; uint32_t iterations, chains;
    bool may_inline;                                            // few rows (≤ FM_INLINE_WORDS words) may travel in the kernel arguments: the peeled launch only
    int64_t ops, vectors, stored; ProfileTag tag;               // operations executed; vectors of n elements moved, and those written among them; the profile's tag
    // a fused reduction of n_red values per row (red == nullptr: none): begun here; to wait for it and to release it is the caller's
    RedLaunch* red = nullptr; int n_red = 0; double shift = 0.0; fmhip_moments* host_moments = nullptr; void* dev_moments = nullptr;
};

// On the stream, in this order: table upload (through the pinned ring), first profiling event, red_begin, launch, second event.
void Engine::launch_row_table(const RowLaunch& l, const std::vector<uint64_t>& table) {
    DevRolledArgs args{};
    args.n = l.n; args.tiles_per_row = (uint32_t)l.tiles; args.row_words = (uint32_t)l.row_words; args.iterations = l.iterations; args.pad = l.chains;
    args.dump = (uint64_t)(uintptr_t)dump_dev_;
    const size_t table_bytes = table.size() * 8;
    const bool inline_rows = l.may_inline && table.size() <= (size_t)FM_INLINE_WORDS;
    const uint64_t* rows_arg = nullptr;
    if (inline_rows) std::memcpy(args.inline_row, table.data(), table_bytes);
    else {                                                      // through the pinned ring
        const size_t ring_off = ring_reserve(table_bytes);
        std::memcpy((char*)ring_host_ + ring_off, table.data(), table_bytes);
        const hipError_t e = hipMemcpyAsync((char*)ring_dev_ + ring_off, (char*)ring_host_ + ring_off, table_bytes, hipMemcpyHostToDevice, stream_);
        if (e != hipSuccess) hip_check(e, (std::string(l.what) + " row table H2D").c_str());
        rows_arg = (const uint64_t*)((char*)ring_dev_ + ring_off);
    }
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (profiling_) { hip_check(hipEventCreate(&ev0), "hipEventCreate"); hip_check(hipEventCreate(&ev1), "hipEventCreate"); hip_check(hipEventRecord(ev0, stream_), "hipEventRecord"); }
    if (l.red) {
        red_begin(*l.red, (int)l.rows, l.n_red, (size_t)l.tiles, l.host_moments, l.dev_moments);
        args.shift = l.shift; args.partials = (double*)l.red->partials; args.results = (double*)l.red->results; args.counters = counters_dev_;
        args.done_flag = const_cast<uint64_t*>(l.red->poll_flag); args.done_value = l.red->done_value;
    }
    void* params[] = { &args, &rows_arg };
    const hipError_t e = hipModuleLaunchKernel(inline_rows ? l.slot->fn_inline : l.slot->fn_table, (unsigned)l.tiles, (unsigned)l.rows, 1, FM_BLOCK, 1, 1, 0, stream_, params, nullptr);
    if (e != hipSuccess) hip_check(e, ("launch " + std::string(l.what) + " kernel").c_str());
    if (profiling_) { hip_check(hipEventRecord(ev1, stream_), "hipEventRecord"); profile_events_.push_back({ ev0, ev1 }); profile_tags_.push_back(l.tag); }
    n_launches_++; n_jit_launches_++; n_rolled_launches_++;
    n_ops_executed_ += l.ops; algorithmic_bytes_ += 4 * l.n * l.vectors; bytes_written_ += 4 * l.n * l.stored;
}

// COMMON ROWS.  What a row computes is a function of the vectors it reads and of its scalars: members whose rows agree in both — the
// parameter sets of a Jacobian batch up to the time step at which their bumped parameter is first used, which read the very same vectors
// because THEIR predecessors were common rows too — are computed once; the others' values are the same vectors (shared storage, copied
// if anybody writes into one in place: make_private).  A row's inputs and scalars are written first (output slots zero), compared with
// the rows before it, and only a row that is new gets output vectors.
static const bool COMMON_ROWS = knob_on("FMHIP_COMMON_ROWS");     // =0: identical rows of a launch are all computed (A/B)

struct Engine::CommonRows {
    size_t rw;                                                  // words per row
    std::unordered_multimap<uint64_t, uint32_t> seen;           // hash of a row → its number
    std::vector<uint64_t> keys;                                 // the rows as they were compared: inputs and scalars, output slots still zero
    // the number of an equal earlier row; or -1, and this one is recorded as row r_new
    int64_t find_or_record(const uint64_t* row, uint32_t r_new) {
        uint64_t h = 0x9e3779b97f4a7c15ull;
        for (size_t w = 0; w < rw; ++w) { h = (h ^ row[w]) * 0xff51afd7ed558ccdull; h ^= h >> 31; }
        auto range = seen.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (std::memcmp(keys.data() + (size_t)it->second * rw, row, rw * 8) == 0) return it->second;
        seen.emplace(h, r_new);
        keys.insert(keys.end(), row, row + rw);
        return -1;
    }
};

// The members of a common row receive the vectors its first member stored (one more reference each).  span: per launch row its outs
// [begin, end); first_of_row: the member that computed it; retarget(c, i, s): s, a copy of the i-th of them, becomes member c's.
template <class Retarget>
void Engine::share_common_rows(std::vector<Stored>& outs, const std::vector<std::pair<size_t, size_t>>& span, const std::vector<uint32_t>& row_of,
                               const std::vector<size_t>& first_of_row, Retarget&& retarget)
{
    if (first_of_row.size() == row_of.size()) return;
    const size_t n_first = outs.size();
    for (size_t c = 0; c < row_of.size(); ++c) {
        const size_t r = row_of[c];
        if (first_of_row[r] == c) continue;
        for (size_t k = span[r].first; k < span[r].second && k < n_first; ++k) { Stored s = outs[k]; s.buf->refs++; retarget(c, k - span[r].first, s); outs.push_back(s); }
    }
}

static uint64_t ptr_of(const Buffer* b) {          // a vector a row reads, as a word of its table
    if (!b) throw Error(FMHIP_ERR_PROGRAM_LIMIT, "a loop kernel reads a value that has not been computed");
    return (uint64_t)(uintptr_t)b->ptr;
}

// One launch for the rolled stretch of every member of a group: row tables by index, launch (always through the ring), commit.
void Engine::run_rolled(const BigPlan::Rolled& ro, std::vector<BigDag>& group, size_t first, size_t count)
{
    const size_t G = ro.global_leaf.size(), CI = ro.carried.size(), CO = ro.final_pos.size(), LI = ro.leaf_in.size(), LO = ro.out_pos.size(), LS = ro.scal_pos.size();
    const size_t R = ro.iterations, P = ro.period, rw = ro.row_words;
    const int64_t n = group[first].n;
    std::vector<uint64_t> table(count * rw, 0);
    std::vector<Stored> outs;
    outs.reserve(count * (R * LO + CO));
    try {
        for (size_t c = 0; c < count; ++c) {
            BigDag& big = group[first + c];
            auto fresh = [&](size_t pos) { Buffer* b = new_buffer(n); outs.push_back({ &big, pos, nullptr, b }); return (uint64_t)(uintptr_t)b->ptr; };
            uint64_t* row = table.data() + c * rw;
            for (size_t k = 0; k < G; ++k) row[k] = ptr_of(big.leaves[(size_t)ro.global_leaf[k]]->buf);
            for (size_t k = 0; k < CI; ++k) row[G + k] = ptr_of(big.value(ro.begin - P + ro.carried[k]));       // the iteration before the loop ran as ordinary launches
            float* sc = reinterpret_cast<float*>(row + G + CI + CO + R * (LI + LO));
            for (size_t r = 0; r < R; ++r) {
                uint64_t* ip = row + G + CI + CO + r * (LI + LO);
                const size_t base = ro.begin + r * P;
                for (size_t m = 0; m < LI; ++m) ip[m] = ptr_of(big.leaves[(size_t)ro.iter_leaf[r * LI + m]]->buf);
                for (size_t m = 0; m < LO; ++m) ip[LI + m] = fresh(base + ro.out_pos[m]);
                for (size_t m = 0; m < LS; ++m) sc[r * LS + m] = big.scalar_at(base + ro.scal_pos[m]);
            }
            for (size_t k = 0; k < CO; ++k) row[G + CI + k] = fresh(ro.begin + (R - 1) * P + ro.final_pos[k]);    // after the per-iteration outputs, in this order
        }
        if (n > 0) {
            const int64_t elems_per_pass = (int64_t)FM_BLOCK * ro.jit->elems;
            const int64_t moved = (int64_t)(G + CI + CO + R * (LI + LO)), written = (int64_t)(CO + R * LO), rows = (int64_t)count;
            launch_row_table({ ro.jit.get(), "rolled", n, (n + elems_per_pass - 1) / elems_per_pass, count, rw, (uint32_t)R, 0, false,
                               (int64_t)(R * P) * rows, moved * rows, written * rows,
                               { (int)(R * P), (int)(G + CI + R * LI), (int)(R * LO + CO), 0, (int)count, 2, n } }, table);
        }
    } catch (...) { for (Stored& o : outs) buffer_unref(o.buf); throw; }
    commit_stored(outs);
}

// The whole component of every member of a group as ONE launch of its peeled kernel (plan_peel): row tables by index (common rows once),
// launch, commit.
void Engine::run_peeled(const BigPlan::Rolled& ro, std::vector<BigDag>& group, size_t first, size_t count, ReduceRequest* rr, std::vector<uint32_t>* row_of_out)
{
    const BigPlan::Rolled::Peeled& pe = ro.peeled;
    const size_t NX = pe.extra_leaf.size(), G = ro.global_leaf.size(), CO = ro.final_pos.size(), NXO = pe.pre_out.size() + pe.post_out.size();
    const size_t LI = ro.leaf_in.size(), LO = ro.out_pos.size(), LS = ro.scal_pos.size(), NS0 = pe.n_pre_scal, NS2 = pe.n_post_scal;
    const size_t R = ro.iterations, P = ro.period, rw = pe.row_words;
    const size_t oG = NX, oCO = oG + G, oXO = oCO + CO, oIT = oXO + NXO;
    const int64_t n = group[first].n;
    std::vector<uint64_t> table(count * rw, 0);
    std::vector<Stored> outs;
    outs.reserve(count * (R * LO + CO + NXO));
    std::vector<uint32_t> row_of(count);
    std::vector<size_t> member_of_row;                          // launch row → the member (offset from `first`) that it computes
    std::vector<std::pair<size_t, size_t>> span;                // launch row → its outs [begin, end)
    const bool dedup = COMMON_ROWS && count > 1 && (!rr || row_of_out);
    CommonRows common{ rw, {}, {} };
    try {
        for (size_t c = 0; c < count; ++c) {
            BigDag& big = group[first + c];
            const size_t r_new = member_of_row.size();
            uint64_t* row = table.data() + r_new * rw;
            std::fill(row, row + rw, (uint64_t)0);
            for (size_t k = 0; k < NX; ++k) row[k] = ptr_of(big.leaves[(size_t)pe.extra_leaf[k]]->buf);
            for (size_t k = 0; k < G; ++k) row[oG + k] = ptr_of(big.leaves[(size_t)ro.global_leaf[k]]->buf);
            float* sc = reinterpret_cast<float*>(row + oIT + R * (LI + LO));
            for (size_t k = 0; k < NS0; ++k) sc[k] = big.scalar_at(pe.pre_scal[k]);
            for (size_t r = 0; r < R; ++r) {
                uint64_t* ip = row + oIT + r * (LI + LO);
                const size_t base = ro.begin + r * P;
                for (size_t m = 0; m < LI; ++m) ip[m] = ptr_of(big.leaves[(size_t)ro.iter_leaf[r * LI + m]]->buf);
                for (size_t m = 0; m < LS; ++m) sc[NS0 + r * LS + m] = big.scalar_at(base + ro.scal_pos[m]);
            }
            for (size_t k = 0; k < NS2; ++k) sc[NS0 + R * LS + k] = big.scalar_at(pe.post_scal[k]);
            const int64_t equal = dedup ? common.find_or_record(row, (uint32_t)r_new) : -1;
            if (equal >= 0) { row_of[c] = (uint32_t)equal; ++n_common_rows_; continue; }
            row_of[c] = (uint32_t)r_new;
            member_of_row.push_back(c);
            const size_t out_begin = outs.size();
            auto fresh = [&](size_t pos) { Buffer* b = new_buffer(n); outs.push_back({ &big, pos, nullptr, b }); return (uint64_t)(uintptr_t)b->ptr; };
            for (size_t k = 0; k < CO; ++k) if (pe.final_store[k]) row[oCO + k] = fresh(ro.begin + (R - 1) * P + ro.final_pos[k]);
            for (size_t k = 0; k < pe.pre_out.size(); ++k) row[oXO + k] = fresh(pe.pre_out[k]);
            for (size_t k = 0; k < pe.post_out.size(); ++k) row[oXO + pe.pre_out.size() + k] = fresh(pe.post_out[k]);
            for (size_t r = 0; r < R; ++r) {
                uint64_t* ip = row + oIT + r * (LI + LO);
                for (size_t m = 0; m < LO; ++m) ip[LI + m] = fresh(ro.begin + r * P + ro.out_pos[m]);
            }
            span.push_back({ out_begin, outs.size() });
        }
        const size_t rows = member_of_row.size();
        table.resize(rows * rw);
        if (n > 0) {
            // Tiles per workgroup: ONE (the kernel derives its stretch from the grid).  Measured against 2 and 4
            // (profiles/round04_peel_tiles_per_workgroup.txt): a workgroup that walks two or four tiles one after the other — a quarter of
            // the partials, arrival counts and lingering keeper waves of a launch that takes the moments of its roots — is SLOWER on every
            // kind of launch (valuation chains 5607 → 5527 → 5424 GB/s, simulation components −2 % and −4 %): these kernels live on the
            // number of independent tiles in flight.  Same moments either way (the reduction tree is defined on the vector, fm_kernel_parts.hpp).
            const int64_t elems_per_pass = (int64_t)FM_BLOCK * pe.jit->elems;
            const int64_t stored = (int64_t)(R * LO + NXO) + std::count(pe.final_store.begin(), pe.final_store.end(), (char)1), read = (int64_t)(NX + G + R * LI);
            RowLaunch l{ rr ? pe.jit_red.get() : pe.jit.get(), "peeled", n, (n + elems_per_pass - 1) / elems_per_pass, rows, rw, (uint32_t)R, 0, true,
                         (int64_t)pe.n_ops * (int64_t)rows, (read + stored) * (int64_t)rows, stored * (int64_t)rows,
                         { (int)pe.n_ops, (int)read, (int)stored, rr ? 1 : 0, (int)rows, 2, n } };
            RedLaunch red;
            std::vector<fmhip_moments> by_row;                  // host moments arrive per ROW; the caller's array is per member
            if (rr) {                           // the kernel with the fused reduction of the root (rr->host_out: one entry per member; rr->dev_out: one slot per row)
                if (rr->host_out && rows != count) by_row.resize(rows);
                l.red = &red; l.n_red = 1; l.shift = rr->shift; l.host_moments = by_row.empty() ? rr->host_out : by_row.data(); l.dev_moments = rr->dev_out;
            }
            try {
                launch_row_table(l, table);
                if (rr) {
                    rr->done = true;
                    if (count == 1 && defer_red_ && !defer_red_->pending && rr->host_out && red.on_host) {
                        red.pending = true; red.batch = 1; red.n_red = 1; red.host = rr->host_out;
                        *defer_red_ = red; red = RedLaunch();      // reduce() waits and releases
                    } else {
                        red_wait(red, (int)rows, 1, l.host_moments);
                        if (!by_row.empty()) for (size_t c = 0; c < count; ++c) rr->host_out[c] = by_row[row_of[c]];
                    }
                }
            } catch (...) { red_release(red); throw; }
            red_release(red);
        }
    } catch (...) { for (Stored& o : outs) buffer_unref(o.buf); throw; }
    if (row_of_out) *row_of_out = row_of;
    share_common_rows(outs, span, row_of, member_of_row, [&](size_t c, size_t, Stored& s) { s.big = &group[first + c]; });
    commit_stored(outs);
}

// The loop of a component shape (detect_loop) and its peeled form (plan_peel), their kernels asked of the specialised tier; nothing runs.
void Engine::plan_loop(BigPlan& plan, const BigDag& g) {
    static const bool ROLL = knob_on("FMHIP_ROLL");
    if (!ROLL) return;
    const OperandTable table(g);
    const std::vector<std::array<int32_t, 3>>& operand = table.operand;
    std::string source; int elems = 0;
    RolledBody body;
    if (!detect_loop(g, operand, plan.rolled, &source, &elems, &body)) return;
    if (plan_peel(g, operand, plan.rolled, body) && jit_mode != FMHIP_JIT_OFF)
        plan.rolled.peeled.jit = jit().request_source(plan.rolled.peeled.source, plan.rolled.peeled.elems, jit_mode == FMHIP_JIT_SYNC);
    if (const char* dump = std::getenv("FMHIP_ROLL_DUMP")) { if (FILE* f = std::fopen(dump, "a")) { std::fputs(source.c_str(), f); std::fputs("\n// ----\n", f); std::fclose(f); } }
    plan.rolled.present = true;
    plan.rolled.source = source; plan.rolled.elems = elems;
    if (jit_mode != FMHIP_JIT_OFF) plan.rolled.jit = jit().request_source(std::move(source), elems, jit_mode == FMHIP_JIT_SYNC);
}

} // namespace fm
