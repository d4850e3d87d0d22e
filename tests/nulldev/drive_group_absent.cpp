// drive_group_absent.cpp — a build of the engine WITHOUT the launchers of group_kernel.hip (no stand-in for them is linked: the weak
// references stay null; the sort's are there) on the TEST-ONLY null device: fmhip_group_sums answers FMHIP_ERR_UNSUPPORTED — after its
// argument checks, which still come first — and never falls back; the definition (the _host twin) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000, m = 7;
        std::vector<float> index((size_t)n), x((size_t)n);
        for (int64_t p = 0; p < n; ++p) { index[(size_t)p] = (float)((p * 37) % 9); x[(size_t)p] = (float)p; }      // 7 and 8 belong to no group
        fmhip_vec vi = 0, vx = 0, longer = 0, out = 0, counts = 0;
        OK(fmhip_vec_create_from_float(index.data(), n, &vi));
        OK(fmhip_vec_create_from_float(x.data(), n, &vx));
        OK(fmhip_vec_create_from_float(x.data(), n - 1, &longer));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        int64_t ungrouped = -7;
        EXPECT(fmhip_group_sums(vi, m, &vx, 5, 1u, &counts, &out, &ungrouped), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_group_sums(vi, 0, &vx, 1, 1u, &counts, &out, &ungrouped), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_group_sums(vi, m, &vx, 1, 0u, &counts, &out, &ungrouped), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_group_sums(vi, m, &longer, 1, 1u, &counts, &out, &ungrouped), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_group_sums(vi, m, &vx, 1, 1u, &counts, &out, &ungrouped), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_group_sums(vi, m, nullptr, 0, 0u, &counts, nullptr, nullptr), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_group_sums(vi, m, nullptr, 0, 0u, nullptr, nullptr, &ungrouped), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || counts != 0 || ungrouped != -7) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        // the definition needs no kernel
        std::vector<float> got((size_t)m), c((size_t)m);
        const float* in[1] = { x.data() }; float* columns[1] = { got.data() };
        OK(fmhip_group_sums_host(index.data(), n, m, in, 1, 1u, c.data(), columns, &ungrouped));
        std::vector<double> want((size_t)m, 0.0); std::vector<int64_t> count((size_t)m, 0); int64_t none = 0;
        for (int64_t p = 0; p < n; ++p) { const int64_t k = (p * 37) % 9; if (k < m) { want[(size_t)k] += (double)p; count[(size_t)k]++; } else ++none; }      // (integers: exact in any order)
        for (int64_t k = 0; k < m; ++k) if (got[(size_t)k] != (float)want[(size_t)k] || c[(size_t)k] != (float)count[(size_t)k]) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)k); std::abort(); }
        if (ungrouped != none) { std::fprintf(stderr, "the ungrouped count is off\n"); std::abort(); }
        OK(fmhip_vec_release(vi)); OK(fmhip_vec_release(vx)); OK(fmhip_vec_release(longer));
        std::printf("cycle %d: group absent done\n", cycle);
        std::fflush(stdout);
    });
}
