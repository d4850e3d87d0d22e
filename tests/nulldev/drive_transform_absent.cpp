// drive_transform_absent.cpp — a build of the engine WITHOUT the launcher of transform_kernel.hip (no stand-in for it is linked: the weak
// reference stays null) on the TEST-ONLY null device: fmhip_transform_option answers FMHIP_ERR_UNSUPPORTED — after its argument checks,
// which still come first — and never falls back; the host-only call needs no kernel; nothing is left behind.
#include <cmath>

#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101) + 60.0f;
        // one node at u = 0 with weight 1/π·… folded so that E = 1: G = 1, the value N·(F − √(FK))
        const double table[3] = { 0.0, 0.0, 0.0 };
        fmhip_vec v = 0, out[3] = { 0, 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &v));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        EXPECT(fmhip_transform_option(table, 0, 0, v, 0.0, nullptr, nullptr, 0, 1.0, 100.0, 3, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_transform_option(table, 1, 0, 0, 100.0, nullptr, nullptr, 0, 1.0, 100.0, 3, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_transform_option(table, 1, 0, v, 0.0, nullptr, nullptr, 0, 1.0, 100.0, 3, out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_transform_option(table, 1, 0, 0, 100.0, nullptr, nullptr, v, 0.0, 100.0, FMHIP_TRANSFORM_DELTA, out), FMHIP_ERR_UNSUPPORTED);
        if (out[0] != 0 || out[1] != 0 || out[2] != 0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        std::vector<float> value((size_t)n, -1.0f);
        float* cols[1] = { value.data() };
        OK(fmhip_transform_option_host(table, 1, 0, a.data(), 0.0, nullptr, nullptr, nullptr, 2.0, n, 100.0, FMHIP_TRANSFORM_VALUE, cols));      // the definition needs no kernel
        for (int64_t p = 0; p < n; ++p) {
            const double want = 2.0 * ((double)a[(size_t)p] - std::sqrt((double)a[(size_t)p] * 100.0));
            if (!(std::fabs((double)value[(size_t)p] - want) <= 1e-5 * (1.0 + std::fabs(want)))) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)p); std::abort(); }
        }
        OK(fmhip_vec_release(v));
        std::printf("cycle %d: transform option absent done\n", cycle);
        std::fflush(stdout);
    });
}
