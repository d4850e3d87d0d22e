// drive_prefix_absent.cpp — a build of the engine WITHOUT the launchers of prefix_kernel.hip (no stand-in for them is linked: the weak
// references stay null) on the TEST-ONLY null device: the three device calls answer FMHIP_ERR_UNSUPPORTED — after their argument checks,
// which still come first — and never fall back; the definition (fmhip_prefix_sums_host) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101);
        fmhip_vec v = 0, out = 0;
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        const int64_t positions[3] = { 0, n - 1, 5 };
        const double thresholds[2] = { 0.5, 1.0 };
        double sums[3] = { -1.0, -1.0, -1.0 }, total = -1.0;
        int64_t where[2] = { -7, -7 };
        EXPECT(fmhip_prefix_sums(v, 2, &out, &total), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_prefix_sums_at(v, positions, 0, sums), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_prefix_search(v, thresholds, 4097, 1, where, sums, &total), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_prefix_sums(v, 0, &out, &total), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_prefix_sums(v, 1, &out, nullptr), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_prefix_sums_at(v, positions, 3, sums), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_prefix_search(v, thresholds, 2, 1, where, sums, &total), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || total != -1.0 || sums[0] != -1.0 || where[0] != -7) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<double> prefix((size_t)n, -1.0);
        OK(fmhip_prefix_sums_host(a.data(), n, prefix.data()));
        double run = 0.0;
        for (int64_t r = 0; r < n; ++r) { run += (double)a[(size_t)r]; if (prefix[(size_t)r] != run) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)r); std::abort(); } }      // integers: every order gives the same bits
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: prefix absent done\n", cycle);
        std::fflush(stdout);
    });
}
