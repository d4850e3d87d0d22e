// drive_block_order_absent.cpp — a build of the engine WITHOUT the launcher of block_order_kernel.hip (no stand-in for it is linked: the weak
// reference stays null) on the TEST-ONLY null device: the two device calls answer FMHIP_ERR_UNSUPPORTED — after their argument checks,
// which still come first — and never fall back; the definitions (the _host calls) need no kernel; nothing is left behind.
#include <algorithm>

#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000, block = 8, m = n / block;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101);
        fmhip_vec v = 0, out = 0, outs[3] = { 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        const int64_t ranks[2] = { 0, 7 }, from[1] = { 0 }, to[1] = { 7 }, outside[1] = { 8 };
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_block_order_statistics(&v, 1, block, ranks, 0, from, to, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_order_statistics(&v, 1, block, outside, 1, from, to, 1, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_order_statistics(&v, 1, 7, ranks, 1, from, to, 0, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_sort(v, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_order_statistics(&v, 1, block, ranks, 2, from, to, 1, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_block_order_statistics(&v, 1, n, ranks, 1, from, to, 0, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_block_sort(v, block, &out), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || outs[0] != 0 || outs[1] != 0 || outs[2] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> got((size_t)(3 * m), -1.f), sorted((size_t)n, -1.f);
        OK(fmhip_block_order_statistics_host(a.data(), n, block, ranks, 2, from, to, 1, got.data()));
        OK(fmhip_block_sort_host(a.data(), n, block, sorted.data()));
        for (int64_t q = 0; q < m; ++q) {
            std::vector<float> s(a.begin() + q * block, a.begin() + (q + 1) * block);
            std::sort(s.begin(), s.end());
            float run = 0.f;
            for (float x : s) run += x;                                                              // integers: every order gives the same bits
            if (got[(size_t)q] != s.front() || got[(size_t)(m + q)] != s.back() || got[(size_t)(2 * m + q)] != run / 8.f || !std::equal(s.begin(), s.end(), sorted.begin() + q * block)) {
                std::fprintf(stderr, "the definition is off at block %lld\n", (long long)q); std::abort();
            }
        }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: block order absent done\n", cycle);
        std::fflush(stdout);
    });
}
