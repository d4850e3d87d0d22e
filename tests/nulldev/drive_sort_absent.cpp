// drive_sort_absent.cpp — a build of the engine WITHOUT the launchers of sort_kernel.hip (no stand-in is linked: the weak references stay
// null) on the TEST-ONLY null device: the four device calls answer FMHIP_ERR_UNSUPPORTED — after their argument checks, which still come
// first — and never fall back; the definition (fmhip_argsort_host) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> a((size_t)n);
        for (int64_t p = 0; p < n; ++p) a[(size_t)p] = (float)((p * 37) % 101);
        fmhip_vec key = 0, shorter = 0, out = 0, outs[2] = { 0, 0 };
        OK(fmhip_vec_create_from_float(a.data(), n, &key));
        OK(fmhip_vec_create_filled(n - 1, 2.0, &shorter));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        std::vector<int64_t> perm((size_t)n, -1), want((size_t)n, -1);
        const fmhip_vec both[2] = { key, key }, bad[2] = { key, shorter };
        const int64_t positions[3] = { 0, n - 1, 5 };
        double elements[3];
        EXPECT(fmhip_sort_by_key(key, both, 9, &out, outs), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_sort_by_key(key, bad, 2, &out, outs), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_vec_read_elements(key, positions, 0, elements), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_sort_by_key(key, both, 2, &out, outs), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_sort_by_key(key, nullptr, 0, &out, nullptr), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_argsort(key, perm.data()), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_rank_scores(key, &out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_vec_read_elements(key, positions, 3, elements), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || outs[0] != 0 || outs[1] != 0 || perm[0] != -1) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        OK(fmhip_argsort_host(a.data(), n, want.data()));
        for (int64_t r = 1; r < n; ++r) {
            const float lo = a[(size_t)want[(size_t)r - 1]], hi = a[(size_t)want[(size_t)r]];
            if (lo > hi || (lo == hi && want[(size_t)r - 1] > want[(size_t)r])) { std::fprintf(stderr, "the definition is out of order at %lld\n", (long long)r); std::abort(); }
        }
        OK(fmhip_vec_release(key)); OK(fmhip_vec_release(shorter));
        std::printf("cycle %d: sort absent done\n", cycle);
        std::fflush(stdout);
    });
}
