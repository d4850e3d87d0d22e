// drive_cross_order_absent.cpp — a build of the engine WITHOUT the launchers of cross_order_kernel.hip (no stand-in for them is linked: the
// weak references stay null) on the TEST-ONLY null device: the two device calls answer FMHIP_ERR_UNSUPPORTED — after their argument checks,
// which still come first — and never fall back; the definitions (the _host calls) need no kernel; nothing is left behind.
#include <algorithm>

#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n), b((size_t)n), c((size_t)n);
        for (int64_t p = 0; p < n; ++p) { a[(size_t)p] = (float)((p * 37) % 101); b[(size_t)p] = (float)((p * 53) % 103); c[(size_t)p] = (float)((p * 71) % 107); }
        fmhip_vec vs[3] = { 0, 0, 0 }, out = 0, outs[4] = { 0, 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &vs[0]));
        OK(fmhip_vec_create_from_float(b.data(), n, &vs[1]));
        OK(fmhip_vec_create_from_float(c.data(), n, &vs[2]));
        const int ranks[2] = { 0, 2 }, outside[1] = { 3 };
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_cross_order_statistics(vs, 3, ranks, 0, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_cross_order_statistics(vs, 3, outside, 1, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_cross_order_statistics(vs, 3, ranks, 2, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_cross_select(0, vs, 3, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_cross_order_statistics(vs, 3, ranks, 2, 3, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_cross_order_statistics(vs, 1, ranks, 1, 1, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_cross_select(vs[0], vs, 3, &out), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || outs[0] != 0 || outs[1] != 0 || outs[2] != 0 || outs[3] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> lo((size_t)n, -1.f), hi((size_t)n, -1.f), lo_at((size_t)n, -1.f), hi_at((size_t)n, -1.f), picked((size_t)n, -1.f);
        const float* in[3] = { a.data(), b.data(), c.data() };
        float* columns[4] = { lo.data(), hi.data(), lo_at.data(), hi_at.data() };
        OK(fmhip_cross_order_statistics_host(in, 3, n, ranks, 2, 3, columns));
        OK(fmhip_cross_select_host(hi_at.data(), in, 3, n, picked.data()));
        for (int64_t p = 0; p < n; ++p) {
            const float x[3] = { a[(size_t)p], b[(size_t)p], c[(size_t)p] };
            const float smallest = std::min(x[0], std::min(x[1], x[2])), largest = std::max(x[0], std::max(x[1], x[2]));
            const int at = (int)hi_at[(size_t)p], low = (int)lo_at[(size_t)p];
            if (lo[(size_t)p] != smallest || hi[(size_t)p] != largest || at < 0 || at > 2 || x[at] != largest || low < 0 || low > 2 || x[low] != smallest || picked[(size_t)p] != largest) {
                std::fprintf(stderr, "the definition is off at path %lld\n", (long long)p); std::abort();
            }
        }
        for (fmhip_vec h : vs) OK(fmhip_vec_release(h));
        std::printf("cycle %d: cross order absent done\n", cycle);
        std::fflush(stdout);
    });
}
