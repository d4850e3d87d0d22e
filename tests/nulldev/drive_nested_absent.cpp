// drive_nested_absent.cpp — a build of the engine WITHOUT the launchers of nested_kernel.hip (no stand-in for them is linked: the weak
// references stay null) on the TEST-ONLY null device: the two device calls answer FMHIP_ERR_UNSUPPORTED — after their argument checks,
// which still come first — and never fall back; the definition (fmhip_block_moments_host) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000, block = 8, m = n / block;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101);
        fmhip_vec v = 0, out = 0, outs[3] = { 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_block_moments(&v, 1, block, 0u, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_moments(&v, 1, 7, 7u, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_vec_repeat(v, 0, 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_block_moments(&v, 1, block, 7u, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_block_moments(&v, 1, n, 2u, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_vec_repeat(v, 2, 3, &out), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || outs[0] != 0 || outs[1] != 0 || outs[2] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> sums((size_t)m, -1.f);
        OK(fmhip_block_moments_host(a.data(), n, block, FMHIP_BLOCK_SUM, sums.data()));
        for (int64_t q = 0; q < m; ++q) {
            float run = 0.f;
            for (int64_t i = 0; i < block; ++i) run += a[(size_t)(q * block + i)];                   // integers: every order gives the same bits
            if (sums[(size_t)q] != run) { std::fprintf(stderr, "the definition is off at block %lld\n", (long long)q); std::abort(); }
        }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: nested absent done\n", cycle);
        std::fflush(stdout);
    });
}
