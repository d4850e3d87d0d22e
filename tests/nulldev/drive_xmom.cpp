// drive_xmom.cpp — drives fmhip_cross_moments through the C-ABI on the TEST-ONLY null device under the sanitizers, on vectors in every state
// a caller can hand over: stored, pending, rows that share storage, the constant 1, the same handle twice and in both lists, 12 + 4 vectors
// (three blocks), with another thread releasing handles of PENDING operands' inputs and other handles while the call waits, under a tiny
// row-table ring (FMHIP_RING_BYTES); then the errors that are found on the host.  Twice, with a shutdown and a re-initialisation in
// between.  FMNULL_DEVICES=N: behind a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked
// about by a thread that does not own them.  The null device computes nothing element-wise (values are whatever the fills left), so only
// the entries that do not depend on values are checked — (ones, ones) = n —; statuses are checked, the sanitizers do the rest.
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V filled(int64_t n, double v) { V h = 0; OK(fmhip_vec_create_filled(n, v, &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

static void ask(const std::vector<V>& x, const std::vector<V>& y, int64_t n) {
    const size_t nx = x.size(), ny = y.size();
    std::vector<double> sums(nx * (nx + 1) / 2 + nx * ny, -1.0);
    OK(fmhip_cross_moments(x.data(), (int)nx, ny ? y.data() : nullptr, (int)ny, sums.data()));
    size_t at = 0;
    for (size_t i = 0; i < nx; ++i) for (size_t j = i; j < nx; ++j, ++at)
        if (x[i] == 0 && x[j] == 0 && sums[at] != (double)n) { std::fprintf(stderr, "(ones, ones) = %g, expected %lld\n", sums[at], (long long)n); std::abort(); }
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 2049;
    V stored = filled(n, 1.5), other = filled(n, 0.5);
    V pending = 0, twin = 0, more = 0;
    OK(fmhip_call_v2s0(FMHIP_OP_ADD, stored, other, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &twin));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &more));              // the same row as `twin`
    std::vector<V> garbage, inputs;
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, other, (double)i, &g)); garbage.push_back(g); }
    // pending operands whose INPUTS are released by another thread during the call: only the call's own handles keep them computable
    std::vector<V> derived;
    for (int i = 0; i < 8; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    const std::vector<V> small = { 0, stored, pending, twin, more, stored };
    std::vector<V> twelve = { 0, stored, pending, twin, more };
    for (int i = 0; i < 7; ++i) twelve.push_back(derived[(size_t)i]);
    const std::vector<V> four = { derived[7], pending, stored, other };
    if (thread_engines) { std::thread asker([&] { ask(small, { pending, stored }, n); ask(twelve, four, n); }); asker.join(); }   // vectors of another thread's engine
    ask(twelve, four, n);                                                   // 16 vectors: three blocks
    ask(small, { pending, stored }, n);                                     // 8 vectors: one block
    ask({ 0, stored, pending, twin, more, stored, other, derived[0], derived[1] }, {}, n);      // 9 x: (0,0) (0,1) (1,1)
    ask({ stored, 0 }, { other, other, other, other }, n);
    ask({ pending }, {}, n);
    releaser.join();
    // a long pending expression (several launches) that is never read
    V chain = stored; OK(fmhip_vec_retain(chain));
    for (int i = 0; i < 90; ++i) { V next = 0; OK(fmhip_call_v2s1(FMHIP_OP_DISCOUNT, chain, other, 0.01 * (i + 1), &next)); rel(chain); chain = next; }
    ask({ 0, chain }, { chain }, n);
    rel(chain);
    // found on the host, before any launch
    double out[256];
    const V thirteen[13] = { stored, stored, stored, stored, stored, stored, stored, stored, stored, stored, stored, stored, stored };
    const V ones[2] = { 0, 0 }, zero_y[1] = { 0 }, five[5] = { stored, stored, stored, stored, stored };
    EXPECT(fmhip_cross_moments(thirteen, 13, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 0, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 2, five, 5, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 2, five, -1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(nullptr, 2, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 2, nullptr, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 2, nullptr, 0, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(ones, 2, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_cross_moments(thirteen, 2, zero_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    V shorter = filled(n - 1, 1.0);
    const V mixed[3] = { stored, 0, shorter };
    EXPECT(fmhip_cross_moments(mixed, 3, nullptr, 0, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_moments(mixed, 2, &shorter, 1, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_cross_moments(&shorter, 1, nullptr, 0, out), FMHIP_OK);
    rel(shorter);
    for (V d : derived) rel(d);
    rel(stored); rel(other); rel(pending); rel(twin); rel(more);
}

int main() {
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: xmom done\n", cycle);
        std::fflush(stdout);
    });
}
