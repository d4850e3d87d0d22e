// drive_xmom_wide.cpp — drives fmhip_cross_moments_wide through the C-ABI on the TEST-ONLY null device under the sanitizers, on vectors in
// every state a caller can hand over: stored, pending, rows that share storage, the constant 1, the same handle twice and in both lists,
// 1 … 64 vectors (one to four groups), with another thread releasing handles of PENDING operands' inputs and other handles while the call
// waits; then the errors that are found on the host.  Twice, with a shutdown and a re-initialisation in between.  FMNULL_DEVICES=N: behind
// a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked about by a thread that does not own
// them.  The null device computes nothing element-wise, so a derived vector holds whatever its storage held; the two FILLED vectors and the
// constant 1 have known values, and the stand-in (null_xmom_wide.cpp) computes the sums where the engine expects them: every entry of S and T
// between those three is checked exactly — v_i·v_j·n, wherever in the lists and groups they stand —, which is a check of the layout the
// engine reads back and of the shard sums; statuses are checked, the sanitizers do the rest.
#include <map>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V filled(int64_t n, double v) { V h = 0; OK(fmhip_vec_create_filled(n, v, &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

static std::map<V, double> known;                                          // handle -> the value every element holds (0: the constant 1)

static void ask(const std::vector<V>& x, const std::vector<V>& y, int64_t n) {
    const size_t nx = x.size(), ny = y.size();
    std::vector<double> sums(nx * (nx + 1) / 2 + nx * ny, -1.0);
    OK(fmhip_cross_moments_wide(x.data(), (int)nx, ny ? y.data() : nullptr, (int)ny, sums.data()));
    auto expect = [&](V a, V b, double got, const char* where, size_t i, size_t j) {
        if (!known.count(a) || !known.count(b)) return;
        const double want = known[a] * known[b] * (double)n;               // multiples of 1/4 below 2^53: exact in any order, over any shards
        if (got != want) { std::fprintf(stderr, "%s[%zu][%zu] = %g, expected %g\n", where, i, j, got, want); std::abort(); }
    };
    size_t at = 0;
    for (size_t i = 0; i < nx; ++i) for (size_t j = i; j < nx; ++j, ++at) expect(x[i], x[j], sums[at], "S", i, j);
    for (size_t i = 0; i < nx; ++i) for (size_t m = 0; m < ny; ++m, ++at) expect(x[i], y[m], sums[at], "T", i, m);
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 2049;
    V stored = filled(n, 1.5), other = filled(n, 0.5);
    known = { { 0, 1.0 }, { stored, 1.5 }, { other, 0.5 } };
    V pending = 0, twin = 0, more = 0;
    OK(fmhip_call_v2s0(FMHIP_OP_ADD, stored, other, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &twin));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &more));              // the same row as `twin`
    std::vector<V> garbage, inputs;
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, other, (double)i, &g)); garbage.push_back(g); }
    // pending operands whose INPUTS are released by another thread during the call: only the call's own handles keep them computable
    std::vector<V> derived;
    for (int i = 0; i < 40; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    std::vector<V> sixty = { 0, stored, pending, twin, more, stored };
    for (int i = 0; i < 40; ++i) sixty.push_back(derived[(size_t)i]);
    while (sixty.size() < 59) sixty.push_back(other);
    sixty.push_back(0);                                                     // the constant again, in the fourth group
    const std::vector<V> four = { derived[7], pending, stored, other };
    const std::vector<V> twenty(sixty.begin(), sixty.begin() + 20);
    if (thread_engines) { std::thread asker([&] { ask(twenty, { pending, stored }, n); ask(sixty, four, n); }); asker.join(); }   // vectors of another thread's engine
    ask(sixty, four, n);                                                    // 64 vectors: four groups, ten tiles
    ask(twenty, { pending, stored }, n);                                    // 22: two groups
    ask({ 0, stored, pending }, std::vector<V>(45, derived[1]), n);         // 48: three groups, dependents across two group boundaries
    ask({ stored, 0 }, std::vector<V>(62, other), n);
    ask({ pending }, {}, n);
    releaser.join();
    // found on the host, before any launch
    std::vector<double> out(64 * 65 / 2 + 64 * 64);
    const std::vector<V> many(65, stored);
    const V ones[2] = { 0, 0 }, zero_y[1] = { 0 };
    EXPECT(fmhip_cross_moments_wide(many.data(), 65, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 60, many.data(), 5, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 2, many.data(), -1, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(nullptr, 2, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 2, nullptr, 1, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 2, nullptr, 0, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(ones, 2, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments_wide(many.data(), 2, zero_y, 1, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    V shorter = filled(n - 1, 1.0);
    const V mixed[3] = { stored, 0, shorter };
    EXPECT(fmhip_cross_moments_wide(mixed, 3, nullptr, 0, out.data()), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_moments_wide(mixed, 2, &shorter, 1, out.data()), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_moments_wide(&shorter, 1, nullptr, 0, out.data()), FMHIP_OK);
    rel(shorter);
    for (V d : derived) rel(d);
    rel(stored); rel(other); rel(pending); rel(twin); rel(more);
}

int main() {
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: xmom wide done\n", cycle);
        std::fflush(stdout);
    });
}
