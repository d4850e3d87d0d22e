// merged_chains_engine.hpp — merged chains (runtime.hpp: merge_families; jit.hpp: RolledBody::chains): components of one loop shape that
// read the same vectors, the shorter ones a suffix of the longest one's, as ONE launch.  Part of runtime.cpp's translation unit (included
// at its end behind loop_engine.hpp, whose row-table launch, common rows and hand-over it uses; nowhere else): Engine member functions in a
// file of their own because runtime.cpp is long enough, and in that translation unit so that every build that lists the engine's sources —
// the library's, the sanitizer builds against the null device — has them without being told.
//
// The 14 swaptions of one exercise date are 14 components of the same loop shape and different length — 14 launches by shape (each with the
// other exercise dates' swaptions of that tenor as its rows), every one of which reads the forward rates of its tenor: L_e[e] 14 times,
// L_e[e + 19] five times, 304 vector reads per exercise date where 61 vectors exist.  A FAMILY is a set of such components, found by
// their vectors: same shape of head, body and tail, the same tail inputs, and the head + loop inputs of each a suffix of the longest
// one's.  One launch per (shape, family size): a row per family, a step per vector of the longest chain, every chain joining at its own
// first step; per chain the same operations on the same operands in the same order as in its own launch, and its moments by the same
// tree — bit-identical results, a fifth of the bytes.  Nothing is assumed about the caller: the family is read off the pending graph.
#include "runtime.hpp"

namespace fm {

static const bool MERGE_SMALL = knob_on("FMHIP_MERGE_SMALL");      // =0: components that fit one launch never join a family

// Is this single-launch component, position by position, head + R iterations of the body + tail of a mergeable loop shape?  (The walk
// that lists its operations — depth first from the root, operands in order — and the schedule of the large components of the same shape
// list a chain the same way; where they do not, the answer is no and the component runs on its own as before.)
const Engine::SmallMatch* Engine::match_small(const Dag& d)
{
    if (!MERGE_SMALL || merge_shapes_.empty()) return nullptr;
    auto known = small_match_.find(d.sig);
    if (known != small_match_.end()) {
        if (known->second.ok) return &known->second;
        if (known->second.shape == (int)merge_shapes_.size()) return nullptr;      // (no, with every shape known today)
    }
    if (small_match_.size() > 4096) small_match_.clear();
    SmallMatch& out = small_match_[d.sig];
    out = SmallMatch();
    out.shape = (int)merge_shapes_.size();                      // (looked at with these shapes known: asked again when another one appears)
    const size_t m = d.order.size(), n_in = d.leaves.size();
    if (d.roots.size() != 1 || d.outs.size() != 1 || m == 0 || d.order.back() != d.roots[0] || d.ops.size() != m) return nullptr;
    for (size_t si = 0; si < merge_shapes_.size() && !out.ok; ++si) {
        const RolledBody& B = merge_shape_bodies_[si];
        const RolledBody::Peel& PL = B.peel;
        const size_t n_pre = PL.pre.size(), n_post = PL.post.size(), P = B.ops.size(), NXa = PL.extra_pre, NXP = PL.extra_post;
        if (m < n_pre + n_post || (m - n_pre - n_post) % P != 0) continue;
        // the tail stores nothing but the component's root, or nothing at all
        if (!(PL.post_out.empty() || (PL.post_out.size() == 1 && PL.post_out[0] + 1 == n_post)) || PL.reduce != "q" + std::to_string(n_post - 1)) continue;
        const size_t R = (m - n_pre - n_post) / P;
        std::vector<int> seq(NXa + R, -1), post(NXP, -1);
        bool ok = true;
        // an operand by name → what it must be here: position of an operation (>= 0), or a sequence / tail vector (checked against the leaf)
        auto check = [&](const RolledBody::Op& op, size_t i, auto&& resolve) {
            const SsaOp& a = d.ops[i];
            UVariant uv{};
            if (!micro_op_for(a.opcode, 0, math_mode, &uv) || uv.uop != op.uop || op_info(a.opcode).scalar != op.scalar) return false;
            const int ids[3] = { a.a, a.b, a.c };
            const std::string* names[3] = { &op.x0, &op.x1, &op.x2 };
            const int pos[3] = { 0, uv.r1_pos, uv.r2_pos };
            for (int k = 0; k < 3; ++k) {
                if (names[k]->empty()) { if (k > 0 && pos[k] >= 0) return false; continue; }
                if (pos[k] < 0 || ids[pos[k]] < 0) return false;
                if (!resolve(*names[k], ids[pos[k]])) return false;
            }
            return true;
        };
        auto is_op = [&](int id, size_t position) { return id >= (int)n_in && (size_t)(id - (int)n_in) == position; };
        auto is_leaf = [&](int id, int& slot) { if (id < 0 || id >= (int)n_in) return false; if (slot < 0) slot = id; return slot == id; };
        for (size_t i = 0; i < n_pre && ok; ++i)
            ok = check(PL.pre[i], i, [&](const std::string& nm, int id) {
                const size_t idx = (size_t)std::atoi(nm.c_str() + 1);
                if (nm[0] == 'x') return idx < NXa && is_leaf(id, seq[idx]);
                if (nm[0] == 'p') return idx < i && is_op(id, idx);
                return false; });
        for (size_t r = 0; r < R && ok; ++r)
            for (size_t q = 0; q < P && ok; ++q) {
                const size_t base = n_pre + r * P;
                ok = check(B.ops[q], base + q, [&](const std::string& nm, int id) {
                    const size_t idx = (size_t)std::atoi(nm.c_str() + 1);
                    if (nm[0] == 'v') return idx < q && is_op(id, base + idx);
                    if (nm[0] == 'c') {
                        if (idx >= B.carried.size()) return false;
                        if (r > 0) return is_op(id, base - P + B.carried[idx]);
                        const std::string& init = PL.carried_init[idx];
                        return init[0] == 'p' && is_op(id, (size_t)std::atoi(init.c_str() + 1)); }
                    if (nm == "l0") return is_leaf(id, seq[NXa + r]);
                    return false; });
            }
        for (size_t i = 0; i < n_post && ok; ++i) {
            const size_t base = n_pre + R * P;
            ok = check(PL.post[i], base + i, [&](const std::string& nm, int id) {
                const size_t idx = (size_t)std::atoi(nm.c_str() + 1);
                if (nm[0] == 'q') return idx < i && is_op(id, base + idx);
                if (nm[0] == 'x') return idx >= NXa && idx < NXa + NXP && is_leaf(id, post[idx - NXa]);
                if (nm[0] == 'F') {
                    if (idx >= B.final_pos.size()) return false;
                    if (R > 0) return is_op(id, base - P + B.final_pos[idx]);
                    for (size_t c = 0; c < B.carried.size(); ++c)
                        if (B.carried[c] == B.final_pos[idx]) { const std::string& init = PL.carried_init[c]; return init[0] == 'p' && is_op(id, (size_t)std::atoi(init.c_str() + 1)); }
                    return false; }
                return false; });
        }
        // every vector of the sequence is a vector of its own step (the kernel loads one per step), every leaf is accounted for
        for (int v : seq) ok = ok && v >= 0;
        for (int v : post) ok = ok && v >= 0;
        if (ok) { std::vector<int> all(seq); all.insert(all.end(), post.begin(), post.end()); std::sort(all.begin(), all.end()); ok = all.size() == n_in && std::adjacent_find(all.begin(), all.end()) == all.end(); }
        if (!ok) continue;
        out.ok = true; out.shape = (int)si; out.R = (uint32_t)R;
        out.seq_leaf.assign(seq.begin(), seq.end()); out.post_leaf.assign(post.begin(), post.end());
    }
    if (!out.ok) { out.shape = (int)merge_shapes_.size(); return nullptr; }
    return &out;
}

// The number of a mergeable loop shape (by its description), registered at its first sight — when its plan is made (plan_peel), so that
// single-launch components of the flush after can be recognised as its chains; -1: the shape has no merged form.
int Engine::merge_shape_index(const std::string& desc)
{
    if (desc.empty()) return -1;
    for (size_t i = 0; i < merge_shapes_.size(); ++i) if (merge_shapes_[i] == desc) return (int)i;
    RolledBody body;
    if (!jit_parse_description(desc, body)) return -1;
    RolledBody probe = body; probe.chains = 2; probe.shared_den = true;
    if (jit_generate_rolled_source(probe).empty()) return -1;
    merge_shapes_.push_back(desc); merge_shape_bodies_.push_back(std::move(body));
    return (int)merge_shapes_.size() - 1;
}

// What the parts of merge_families share: the candidate chains of a flush, their families and launches, and where a chain's vectors and
// scalars are.  A chain is a large component (group, member: its plan says where they are) or a small one (its group's match does).
struct Engine::MergeContext {
    struct Chain { size_t group, member; BigPlan* plan; int shape; Node* root; uint32_t steps, R; const float* last; bool small; };
    struct Shape { const RolledBody* body = nullptr; size_t NXa = 0, NXP = 0, NS0 = 0, NS2 = 0, LS = 0, NXO = 0, P = 0; std::vector<uint32_t> shared_pre, shared_body; };
    struct Family { std::vector<size_t> chain; };                                  // indices into `chains`, longest first
    struct Launch { std::shared_ptr<JitSlot> slot; std::vector<size_t> rows; };    // a kernel per (shape, family size) and its families
    Engine& e; std::vector<std::vector<BigDag>>& groups; std::vector<SmallGroup>& small;
    std::vector<Chain> chains;
    std::vector<BigPlan*> plan_of_shape;                         // a plan of every shape met in this flush (what its large chains are described by)
    std::unordered_map<int, Shape> shapes;
    std::vector<Family> families; std::vector<Launch> launches;
    std::vector<std::vector<char>> taken, staken;                // per member of a group / small group: 1 = in a family whose kernel is there, 2 = has run

    const Shape& shape_of(int shape) {
        auto it = shapes.find(shape);
        if (it != shapes.end()) return it->second;
        Shape& sh = shapes[shape];
        sh.body = &e.merge_shape_bodies_[(size_t)shape];
        sh.NXa = sh.body->peel.extra_pre; sh.NXP = sh.body->peel.extra_post; sh.NXO = sh.body->peel.post_out.size(); sh.P = sh.body->ops.size();
        for (const RolledBody::Op& op : sh.body->peel.pre) sh.NS0 += op.scalar ? 1 : 0;
        for (const RolledBody::Op& op : sh.body->peel.post) sh.NS2 += op.scalar ? 1 : 0;
        for (const RolledBody::Op& op : sh.body->ops) sh.LS += op.scalar ? 1 : 0;
        jit_merged_shared_scalars(*sh.body, sh.shared_pre, sh.shared_body);
        return sh;
    }
    const Chain& lead(const Family& f) const { return chains[f.chain[0]]; }
    BigDag& big(const Chain& c) const { return groups[c.group][c.member]; }
    const Dag& dag(const Chain& c) const { return small[c.group].members[c.member]; }
    char& mark(const Chain& c) { return c.small ? staken[c.group][c.member] : taken[c.group][c.member]; }
    int64_t chain_n(const Chain& c) const { return c.small ? dag(c).outs[0]->n : big(c).n; }
    static const float* vec_ptr(const Node* leaf) { return leaf->buf ? leaf->buf->ptr : nullptr; }
    // the vector a chain reads at step i of its own sequence (head inputs first, then one per iteration); the vectors of its tail
    const float* seq_ptr(const Chain& c, const Shape& sh, size_t i) const {
        if (c.small) return vec_ptr(dag(c).leaves[(size_t)small[c.group].match->seq_leaf[i]]);
        const BigPlan::Rolled& ro = c.plan->rolled;
        return vec_ptr(big(c).leaves[(size_t)(i < sh.NXa ? ro.peeled.extra_leaf[i] : ro.iter_leaf[(i - sh.NXa) * ro.leaf_in.size()])]);
    }
    const float* post_ptr(const Chain& c, const Shape& sh, size_t x) const {
        if (c.small) return vec_ptr(dag(c).leaves[(size_t)small[c.group].match->post_leaf[x]]);
        return vec_ptr(big(c).leaves[(size_t)c.plan->rolled.peeled.extra_leaf[sh.NXa + x]]);
    }
    // scalar number i of the chain's head / of iteration `it` / of its tail, in the order of the operations
    float pre_scalar(const Chain& c, size_t i) const { return c.small ? dag(c).scalars[i] : big(c).scalar_at(c.plan->rolled.peeled.pre_scal[i]); }
    float body_scalar(const Chain& c, const Shape& sh, size_t it, size_t i) const {
        if (c.small) return dag(c).scalars[sh.NS0 + it * sh.LS + i];
        const BigPlan::Rolled& ro = c.plan->rolled;
        return big(c).scalar_at(ro.begin + it * ro.period + ro.scal_pos[i]);
    }
    float post_scalar(const Chain& c, const Shape& sh, size_t i) const { return c.small ? dag(c).scalars[sh.NS0 + (size_t)c.R * sh.LS + i] : big(c).scalar_at(c.plan->rolled.peeled.post_scal[i]); }
    // the bits of the scalar the shared denominators of a family stand for, as its longest chain has it (0: the shape shares none)
    uint32_t shared_bits(const Chain& lead, const Shape& sh) const {
        float s_star = 0.f;
        if (!sh.shared_pre.empty()) s_star = pre_scalar(lead, sh.shared_pre[0]);
        else if (!sh.shared_body.empty() && lead.R > 0) s_star = body_scalar(lead, sh, 0, sh.shared_body[0]);
        uint32_t bits; std::memcpy(&bits, &s_star, 4);
        return bits;
    }
    size_t section_words(const Chain& c, const Shape& sh) const { return sh.NXO + (sh.NS0 + (size_t)c.R * sh.LS + sh.NS2 + 1) / 2; }
    // A family's row but for its output slots: [steps T of the longest chain] [per chain: its first step | the offset of its section << 32]
    // [the T vectors] [the tail's vectors] [the shared scalar] [per chain a section: output slots, scalars]
    void fill_row(uint64_t* row, const Family& fam, const Shape& sh) const {
        const Chain& longest = lead(fam);
        const size_t K = fam.chain.size(), T = longest.steps;
        row[0] = (uint64_t)T;
        for (size_t t = 0; t < T; ++t) row[1 + K + t] = (uint64_t)(uintptr_t)seq_ptr(longest, sh, t);
        for (size_t x = 0; x < sh.NXP; ++x) row[1 + K + T + x] = (uint64_t)(uintptr_t)post_ptr(longest, sh, x);
        row[1 + K + T + sh.NXP] = shared_bits(longest, sh);
        size_t at = 1 + K + T + sh.NXP + 1;
        for (size_t k = 0; k < K; ++k) {
            const Chain& c = chains[fam.chain[k]];
            row[1 + k] = (uint64_t)(T - c.steps) | ((uint64_t)at << 32);
            float* sc = reinterpret_cast<float*>(row + at + sh.NXO);
            for (size_t i = 0; i < sh.NS0; ++i) sc[i] = pre_scalar(c, i);
            for (size_t it = 0; it < c.R; ++it)
                for (size_t m = 0; m < sh.LS; ++m) sc[sh.NS0 + it * sh.LS + m] = body_scalar(c, sh, it, m);
            for (size_t i = 0; i < sh.NS2; ++i) sc[sh.NS0 + (size_t)c.R * sh.LS + i] = post_scalar(c, sh, i);
            at += section_words(c, sh);
        }
    }
    // the one value a chain stores is its root
    Stored stored(const Chain& c, Buffer* b) const { return c.small ? Stored{ nullptr, 0, c.root, b } : Stored{ &big(c), (size_t)c.plan->rolled.peeled.post_out[0], nullptr, b }; }
};

void Engine::merge_families(std::vector<std::vector<BigDag>>& groups, std::vector<SmallGroup>& small) {
    if (!MERGE_CHAINS || !want_root_moments_ || jit_mode == FMHIP_JIT_OFF) return;
    MergeContext mc{ *this, groups, small };
    merge_collect_large(mc);
    merge_collect_small(mc);
    if (mc.chains.size() < 2) return;
    merge_form_families(mc);
    if (mc.families.empty()) return;
    merge_request_kernels(mc);
    if (!merge_mark_whole_sets(mc)) return;
    for (size_t l = 0; l < mc.launches.size(); ++l) merge_run_launch(mc, l);
    merge_remove_run(mc);
}

// The candidates among the large components: a mergeable peeled plan, a single root whose moments this flush takes, its last vector there.
void Engine::merge_collect_large(MergeContext& mc) {
    for (size_t gi = 0; gi < mc.groups.size(); ++gi) {
        std::vector<BigDag>& g = mc.groups[gi];
        if (g.empty() || g[0].described() || g[0].n <= 0) continue;
        auto planned = plan_cache_.find(g[0].hash);
        if (planned == plan_cache_.end() || planned->second.sig != g[0].sig) continue;
        BigPlan& plan = planned->second;
        BigPlan::Rolled& ro = plan.rolled;
        BigPlan::Rolled::Peeled& pe = ro.peeled;
        if (!ro.present || !pe.present || pe.desc_red.empty() || pe.elems != 8) continue;
        if (pe.mergeable < 0) pe.mergeable = merge_shape_index(pe.desc_red) >= 0 ? 1 : 0;
        if (!pe.mergeable) continue;
        const int shape = merge_shape_index(pe.desc_red);
        if (shape < 0) continue;
        if ((size_t)((g[0].n + FM_UNIT_ELEMS - 1) / FM_UNIT_ELEMS) > (size_t)FM_SPAN_UNITS * 65536) continue;
        if (mc.plan_of_shape.size() <= (size_t)shape) mc.plan_of_shape.resize((size_t)shape + 1, nullptr);
        if (!mc.plan_of_shape[(size_t)shape]) mc.plan_of_shape[(size_t)shape] = &plan;
        const uint32_t steps = (uint32_t)(merge_shape_bodies_[(size_t)shape].peel.extra_pre + ro.iterations);
        for (size_t mi = 0; mi < g.size(); ++mi) {
            const BigDag& b = g[mi];
            Node* r = single_root(b, g[0]);
            if (!r || r->moments_blocked || (plan.discards_root && !r->discard) || r->buf) continue;
            const int32_t last_leaf = ro.iter_leaf[(size_t)(ro.iterations - 1) * ro.leaf_in.size()];
            const Buffer* lb = b.leaves[(size_t)last_leaf]->buf;
            if (!lb) continue;
            mc.chains.push_back({ gi, mi, &plan, shape, r, steps, ro.iterations, lb->ptr, false });
        }
    }
}

// … and among the components that fit one launch (match_small), where a large chain of their shape is there to carry them.
void Engine::merge_collect_small(MergeContext& mc) {
    for (size_t gi = 0; gi < mc.small.size(); ++gi) {
        SmallGroup& sg = mc.small[gi];
        if (!sg.match || sg.members.empty()) continue;
        const int shape = sg.match->shape;
        if ((size_t)shape >= mc.plan_of_shape.size() || !mc.plan_of_shape[(size_t)shape]) continue;      // no large chain of this shape in this flush: nobody to join
        const RolledBody& body = merge_shape_bodies_[(size_t)shape];
        const bool stores_root = !body.peel.post_out.empty();
        const uint32_t steps = (uint32_t)(body.peel.extra_pre + sg.match->R);
        for (size_t mi = 0; mi < sg.members.size(); ++mi) {
            const Dag& d = sg.members[mi];
            if (d.outs.size() != 1 || d.leaves.size() != sg.proto.leaves.size() || d.outs[0]->n <= 0) continue;
            Node* r = d.outs[0];
            // (as run_dags: a root that is held; given up — and held by nobody else, a copy's root but by its group — exactly when the shape stores nothing)
            const bool given_up = r->discard && r->refs_int == ((r->rep_id && r->rep_copy && replica_of(r)) ? 1 : 0);
            if (r->moments_blocked || r->buf || r->refs_ext <= 0 || (stores_root ? r->discard : !given_up)) continue;
            const Buffer* lb = d.leaves[(size_t)sg.match->seq_leaf.back()]->buf;
            if (!lb) continue;
            mc.chains.push_back({ gi, mi, mc.plan_of_shape[(size_t)shape], shape, r, steps, sg.match->R, lb->ptr, true });
        }
    }
}

// Layers and families.  The candidates are sorted by (shape, last vector), longest first.  Within a stretch of the same shape and last
// vector, those whose whole sequence is a suffix of the longest one's and whose tail inputs and shared scalars agree with it form
// families of at most 16 (a family of small components only has nobody to carry it: skipped).  Chains of the SAME length that end in the
// same vector — the same product valued for several parameter sets whose simulations were common rows up to this exercise date
// (run_peeled) — belong to different families: the m-th chain of every length forms layer m; the layers are rows of one launch (and,
// reading the same vectors with the same scalars, one common row of it).
void Engine::merge_form_families(MergeContext& mc) {
    using Chain = MergeContext::Chain;
    std::vector<Chain>& chains = mc.chains;
    std::sort(chains.begin(), chains.end(), [&](const Chain& a, const Chain& b) {
        if (a.shape != b.shape) return a.shape < b.shape;
        if (a.last != b.last) return a.last < b.last;
        if (a.steps != b.steps) return a.steps > b.steps;
        if (a.small != b.small) return !a.small;
        if (a.group != b.group) return a.group < b.group;
        return a.member < b.member;
    });
    auto families_of_layer = [&](const std::vector<size_t>& layer) {
        const Chain& lead = chains[layer[0]];
        if (lead.small) return;
        const MergeContext::Shape& sh = mc.shape_of(lead.shape);
        const uint32_t want = mc.shared_bits(lead, sh);
        auto same = [&](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u == want; };
        MergeContext::Family fam;
        for (size_t q : layer) {
            const Chain& c = chains[q];
            bool ok = mc.chain_n(c) == mc.chain_n(lead);
            for (size_t x = 0; ok && x < sh.NXP; ++x) { const float* p = mc.post_ptr(c, sh, x); ok = p != nullptr && p == mc.post_ptr(lead, sh, x); }
            const size_t shift = lead.steps - c.steps;
            for (size_t t = 0; ok && t < c.steps; ++t) { const float* p = mc.seq_ptr(c, sh, t); ok = p != nullptr && p == mc.seq_ptr(lead, sh, shift + t); }
            // every scalar the shared denominators stand for carries the same bits
            for (uint32_t sl : sh.shared_pre) ok = ok && same(mc.pre_scalar(c, sl));
            for (size_t r = 0; ok && r < c.R; ++r) for (uint32_t sl : sh.shared_body) ok = ok && same(mc.body_scalar(c, sh, r, sl));
            if (!ok) continue;
            fam.chain.push_back(q);
            if (fam.chain.size() == 16) { mc.families.push_back(std::move(fam)); fam = MergeContext::Family(); }
        }
        if (fam.chain.size() >= 2) mc.families.push_back(std::move(fam));
    };
    for (size_t i = 0; i < chains.size();) {
        size_t j = i + 1;
        while (j < chains.size() && chains[j].last == chains[i].last && chains[j].shape == chains[i].shape) ++j;
        std::vector<std::vector<size_t>> layers;
        size_t occurrence = 0;
        for (size_t q = i; q < j; ++q) {
            occurrence = (q > i && chains[q].steps == chains[q - 1].steps) ? occurrence + 1 : 0;
            if (layers.size() <= occurrence) layers.resize(occurrence + 1);
            layers[occurrence].push_back(q);
        }
        for (const std::vector<size_t>& layer : layers) families_of_layer(layer);
        i = j;
    }
    // (after a split at 16 the later part is a family of its own: its first chain is its longest, the others suffixes of it)
    mc.families.erase(std::remove_if(mc.families.begin(), mc.families.end(), [&](const MergeContext::Family& f) { return f.chain.size() < 2 || mc.lead(f).small; }), mc.families.end());
}

// Kernels: one per (shape, family size); a family whose kernel does not exist yet runs as before.
void Engine::merge_request_kernels(MergeContext& mc) {
    std::unordered_map<uint64_t, size_t> launch_of;
    for (size_t f = 0; f < mc.families.size(); ++f) {
        const int shape = mc.lead(mc.families[f]).shape;
        const size_t K = mc.families[f].chain.size();
        const uint64_t lkey = ((uint64_t)shape << 8) | K;
        auto known = launch_of.find(lkey);
        if (known == launch_of.end()) {
            std::shared_ptr<JitSlot>& slot = merged_kernels_[merge_shapes_[(size_t)shape] + " chains " + std::to_string(K) + " sden 1"];
            kernel_ready(slot, [&] {
                RolledBody body = merge_shape_bodies_[(size_t)shape];
                body.chains = (uint32_t)K; body.shared_den = true;
                std::string source = jit_generate_rolled_source(body);
                if (!source.empty()) jit().record(jit_describe(body));
                return source; }, 8);
            if (!slot) continue;
            known = launch_of.emplace(lkey, mc.launches.size()).first;
            mc.launches.push_back({ slot, {} });
        }
        mc.launches[known->second].rows.push_back(f);
    }
}

// The original of a replicated component and its copies go together or not at all: a copy left behind would have nobody to carry its
// order (run_plan, run_dags).  Marks the members of every family whose kernel is there; false — nothing is merged in this flush — if any
// such set is split.
bool Engine::merge_mark_whole_sets(MergeContext& mc) {
    for (const std::vector<BigDag>& g : mc.groups) mc.taken.emplace_back(g.size(), 0);
    for (const SmallGroup& sg : mc.small) mc.staken.emplace_back(sg.members.size(), 0);
    for (const MergeContext::Launch& l : mc.launches) {
        if (!l.slot || l.slot->state.load(std::memory_order_acquire) != JitSlot::READY) continue;
        for (size_t f : l.rows) for (size_t q : mc.families[f].chain) mc.mark(mc.chains[q]) = 1;
    }
    auto whole = [](const auto& members, const std::vector<char>& t, auto&& is_copy) {
        for (size_t mi = 0; mi < members.size(); ++mi) {
            if (is_copy(members[mi])) continue;
            for (size_t q = mi + 1; q < members.size() && is_copy(members[q]); ++q) if (t[q] != t[mi]) return false;
        }
        return true;
    };
    for (size_t gi = 0; gi < mc.groups.size(); ++gi) if (!whole(mc.groups[gi], mc.taken[gi], [](const BigDag& b) { return b.described(); })) return false;
    // (a small copy that exists as a description: vectors, outputs and scalars only)
    for (size_t gi = 0; gi < mc.small.size(); ++gi) if (!whole(mc.small[gi].members, mc.staken[gi], [](const Dag& d) { return d.order.empty(); })) return false;
    return true;
}

// The families of one kernel, rows_per_launch per launch.
void Engine::merge_run_launch(MergeContext& mc, size_t launch) {
    const MergeContext::Launch& l = mc.launches[launch];
    if (!l.slot || l.slot->state.load(std::memory_order_acquire) != JitSlot::READY || l.rows.empty()) return;
    const MergeContext::Chain& first = mc.lead(mc.families[l.rows[0]]);
    const MergeContext::Shape& sh = mc.shape_of(first.shape);
    const size_t K = mc.families[l.rows[0]].chain.size();
    const int64_t n = mc.chain_n(first);
    size_t rw = 0;
    for (size_t f : l.rows) {
        size_t w = 1 + K + mc.lead(mc.families[f]).steps + sh.NXP + 1;
        for (size_t q : mc.families[f].chain) w += mc.section_words(mc.chains[q], sh);
        rw = std::max(rw, w);
    }
    const size_t max_rows = rows_per_launch(rw);
    if (max_rows == 0) return;
    // (rows of one launch have vectors of one length: families are looked for within a flush, whose components of a shape and length
    // share a group; a launch over rows of another length would be a different grid)
    std::vector<size_t> rows_n;
    for (size_t f : l.rows) if (mc.chain_n(mc.lead(mc.families[f])) == n) rows_n.push_back(f);
    for (size_t off = 0; off < rows_n.size(); off += max_rows)
        merge_run_batch(mc, launch, std::vector<size_t>(rows_n.begin() + off, rows_n.begin() + std::min(rows_n.size(), off + max_rows)), rw);
}

// One launch over a batch of families (rows of rw words): the row table with common rows once — families that read the same vectors with
// the same scalars, the parameter sets of a Jacobian batch at an exercise date before their bumped parameter matters, are ONE row; their
// chains share moments and stored values —, the launch, the moments onto the chains' roots, commit.  A launch that cannot get arena
// slots for its moments releases its outputs and leaves its families to run as before.
void Engine::merge_run_batch(MergeContext& mc, size_t launch, const std::vector<size_t>& batch, size_t rw) {
    const size_t count = batch.size(), K = mc.families[batch[0]].chain.size();
    const MergeContext::Chain& first = mc.lead(mc.families[batch[0]]);
    const MergeContext::Shape& sh = mc.shape_of(first.shape);
    const int64_t n = mc.chain_n(first);
    std::vector<uint64_t> table(count * rw, 0);
    std::vector<Stored> outs;
    size_t n_ops = 0, n_vec_in = 0;
    RootMoments along;
    RedLaunch red;
    std::vector<uint32_t> row_of(count);
    std::vector<size_t> family_of_row;                           // launch row → index into the batch
    std::vector<std::pair<size_t, size_t>> out_span;             // launch row → its outs [begin, end)
    CommonRows common{ rw, {}, {} };
    try {
        for (size_t r = 0; r < count; ++r) {
            const MergeContext::Family& fam = mc.families[batch[r]];
            const size_t r_new = family_of_row.size();
            uint64_t* row = table.data() + r_new * rw;
            std::fill(row, row + rw, (uint64_t)0);
            mc.fill_row(row, fam, sh);
            const int64_t equal = COMMON_ROWS && count > 1 ? common.find_or_record(row, (uint32_t)r_new) : -1;
            if (equal >= 0) { row_of[r] = (uint32_t)equal; ++n_common_rows_; continue; }
            row_of[r] = (uint32_t)r_new;
            family_of_row.push_back(r);
            n_vec_in += mc.lead(fam).steps + sh.NXP;
            const size_t out_begin = outs.size();
            for (size_t k = 0; k < K; ++k) {
                const MergeContext::Chain& c = mc.chains[fam.chain[k]];
                uint64_t* sec = row + (size_t)(row[1 + k] >> 32);
                for (size_t m = 0; m < sh.NXO; ++m) { Buffer* nb = new_buffer(n); outs.push_back(mc.stored(c, nb)); sec[m] = (uint64_t)(uintptr_t)nb->ptr; }
                n_ops += sh.body->peel.pre.size() + (size_t)c.R * sh.P + sh.body->peel.post.size();
            }
            out_span.push_back({ out_begin, outs.size() });
        }
        const size_t launch_rows = family_of_row.size();
        table.resize(launch_rows * rw);
        if (!along.open(*this, launch_rows * K)) { for (Stored& o : outs) buffer_unref(o.buf); return; }
        RowLaunch l{ mc.launches[launch].slot.get(), "merged", n, (n + FM_UNIT_ELEMS - 1) / FM_UNIT_ELEMS, launch_rows, rw, 0, (uint32_t)K, false,
                     (int64_t)n_ops, (int64_t)(n_vec_in + outs.size()), (int64_t)outs.size(),
                     { (int)(n_ops / launch_rows), (int)(n_vec_in / launch_rows), (int)(K * sh.NXO), (int)K, (int)launch_rows, 4, n } };
        l.red = &red; l.n_red = (int)K; l.host_moments = along.host(); l.dev_moments = along.dev();
        launch_row_table(l, table);
        n_merged_launches_++; n_merged_chains_ += (int64_t)(count * K);
        red_wait(red, (int)launch_rows, (int)K, l.host_moments);
    } catch (...) { red_release(red); for (Stored& o : outs) buffer_unref(o.buf); throw; }
    red_release(red);
    share_common_rows(outs, out_span, row_of, family_of_row, [&](size_t r, size_t i, Stored& s) {
        s = mc.stored(mc.chains[mc.families[batch[r]].chain[i / std::max<size_t>(1, sh.NXO)]], s.buf); });
    // the moments go to the chains' roots; stored values become vectors; expressions are dismantled
    for (size_t r = 0; r < count; ++r)
        for (size_t k = 0; k < K; ++k) along.deliver(mc.chains[mc.families[batch[r]].chain[k]].root, (size_t)row_of[r] * K + k);
    commit_stored(outs);
    for (size_t r = 0; r < count; ++r)
        for (size_t q : mc.families[batch[r]].chain) {
            const MergeContext::Chain& c = mc.chains[q];
            if (sh.NXO == 0 && !c.root->buf) give_up_value(c.root);
            if (!c.small) TempGuard::drop(this, mc.big(c));
            mc.mark(c) = 2;                                             // has run
        }
}

// What has run leaves its group (the others keep their order: the first member of a group carries the order for its copies).
void Engine::merge_remove_run(MergeContext& mc) {
    auto keep_rest = [](auto& members, const std::vector<char>& t) {
        if (std::find(t.begin(), t.end(), (char)2) == t.end()) return;
        std::remove_reference_t<decltype(members)> rest;
        for (size_t mi = 0; mi < members.size(); ++mi) if (t[mi] != 2) rest.push_back(std::move(members[mi]));
        members.swap(rest);
    };
    for (size_t gi = 0; gi < mc.groups.size(); ++gi) keep_rest(mc.groups[gi], mc.taken[gi]);
    for (size_t gi = 0; gi < mc.small.size(); ++gi) keep_rest(mc.small[gi].members, mc.staken[gi]);
}

} // namespace fm
