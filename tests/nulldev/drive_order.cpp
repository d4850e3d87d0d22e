// drive_order.cpp — drives the engine's order-statistics calls (fmhip_select_ranks_batch, fmhip_rank_sums_batch, fmhip_count_not_above)
// through the C-ABI on the TEST-ONLY null device under the sanitizers, on vectors in every state a caller can hand over: stored, pending,
// deferred candidates that share a row (storage that may be shared: common rows), with another thread releasing other handles while
// the passes wait, under a tiny row-table ring (FMHIP_RING_BYTES); then the errors that are found on the host.  Twice, with a shutdown
// and a re-initialisation in between.  FMNULL_DEVICES=N: behind a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller
// thread, the vectors asked about by a thread that does not own them.  Nothing is computed: statuses are checked, the sanitizers do the rest.
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V filled(int64_t n, double v) { V h = 0; OK(fmhip_vec_create_filled(n, v, &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

static void ask(const V* batch, int count, int64_t n) {
    const int64_t ranks[11] = { 0, n / 2, n - 1, 1, 2, 3, 4, 5, 6, 7, 8 };            // more than eight ranks: two rounds of passes
    std::vector<double> values((size_t)count * 11), sums((size_t)count);
    OK(fmhip_select_ranks_batch(batch, count, ranks, 11, values.data()));
    OK(fmhip_rank_sums_batch(batch, count, 10, n - 10, sums.data()));
    OK(fmhip_rank_sums_batch(batch, count, 7, 7, sums.data()));
    const double bounds[5] = { 0.5, -1.0, __builtin_nan(""), 2.0, 0.5 };
    int64_t counts[5];
    for (int k = 0; k < count; ++k) { OK(fmhip_count_not_above(batch[k], bounds, 5, counts)); if (counts[2] != 0) std::abort(); }
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 2049;
    V stored = filled(n, 1.5), other = filled(n, 0.5);
    V pending = 0, twin = 0, more = 0;
    OK(fmhip_call_v2s0(FMHIP_OP_ADD, stored, other, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &twin));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &more));              // the same row as `twin`
    std::vector<V> garbage;
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, other, (double)i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : garbage) OK(fmhip_vec_release(g)); });       // released by another thread while the passes run
    const V batch[4] = { stored, pending, twin, more };
    if (thread_engines) { std::thread asker([&] { ask(batch, 4, n); }); asker.join(); }   // vectors of another thread's engine
    ask(batch, 4, n);
    ask(&pending, 1, n);
    releaser.join();
    // a pending expression asked for without ever being read, a long one (several launches)
    V chain = stored; OK(fmhip_vec_retain(chain));
    for (int i = 0; i < 90; ++i) { V next = 0; OK(fmhip_call_v2s1(FMHIP_OP_DISCOUNT, chain, other, 0.01 * (i + 1), &next)); rel(chain); chain = next; }
    ask(&chain, 1, n);
    rel(chain);
    // found on the host, before any launch
    double value = 0.0; int64_t count_out = 0;
    const int64_t beyond[1] = { n }, negative[1] = { -1 }, first[1] = { 0 };
    EXPECT(fmhip_select_ranks_batch(batch, 4, beyond, 1, &value), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_select_ranks_batch(batch, 4, negative, 1, &value), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_select_ranks_batch(batch, 0, first, 1, &value), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_rank_sums_batch(batch, 1, 5, 4, &value), FMHIP_ERR_INVALID_ARGUMENT);
    const double bound[1] = { 0.0 };
    EXPECT(fmhip_count_not_above(stored, bound, 0, &count_out), FMHIP_ERR_INVALID_ARGUMENT);
    V shorter = filled(n - 1, 1.0);
    const V mixed[2] = { stored, shorter };
    EXPECT(fmhip_select_ranks_batch(mixed, 2, first, 1, &value), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_select_ranks_batch(&shorter + 0, 1, first, 1, &value), FMHIP_OK);
    rel(shorter);
    rel(stored); rel(other); rel(pending); rel(twin); rel(more);
}

int main() {
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: order done\n", cycle);
        std::fflush(stdout);
    });
}
