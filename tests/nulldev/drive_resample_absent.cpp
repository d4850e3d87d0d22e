// drive_resample_absent.cpp — a build of the engine WITHOUT the launcher of resample_kernel.hip (no stand-in for it is linked: the weak
// reference stays null) on the TEST-ONLY null device: fmhip_resample answers FMHIP_ERR_UNSUPPORTED — after its argument checks, which
// still come first — and never falls back; the definition (fmhip_resample_host) needs no kernel; nothing is left behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000, m = 700;
        std::vector<float> w((size_t)n), x((size_t)n), u((size_t)m, 0.25f);
        for (int64_t p = 0; p < n; ++p) { w[(size_t)p] = (float)((p * 37) % 101); x[(size_t)p] = (float)p; }
        fmhip_vec vw = 0, vx = 0, vu = 0, out = 0, ancestors = 0;
        OK(fmhip_vec_create_from_float(w.data(), n, &vw));
        OK(fmhip_vec_create_from_float(x.data(), n, &vx));
        OK(fmhip_vec_create_from_float(u.data(), m, &vu));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        double total = -1.0;
        EXPECT(fmhip_resample(vw, 3, m, 0.5, 0, &vx, 1, &out, &ancestors, &total), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_SYSTEMATIC, m, 1.0, 0, &vx, 1, &out, &ancestors, &total), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_MULTINOMIAL, m + 1, 0.0, vu, &vx, 1, &out, &ancestors, &total), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_SYSTEMATIC, m, 0.5, 0, &vx, 1, &out, &ancestors, &total), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_STRATIFIED, m, 0.0, vu, nullptr, 0, nullptr, &ancestors, nullptr), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_resample(0, FMHIP_RESAMPLE_MULTINOMIAL, m, 0.0, vu, &vx, 1, &out, nullptr, &total), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || ancestors != 0 || total != -1.0) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        // the definition needs no kernel: integer weights, every order of summation gives the same bits — a linear scan is the check
        std::vector<float> got((size_t)m);
        std::vector<int64_t> a((size_t)m, -7);
        const float* in[1] = { x.data() }; float* columns[1] = { got.data() };
        OK(fmhip_resample_host(w.data(), n, FMHIP_RESAMPLE_SYSTEMATIC, m, 0.5, nullptr, in, 1, columns, a.data(), &total));
        double sum = 0.0;
        for (float f : w) sum += (double)f;
        if (total != sum) { std::fprintf(stderr, "the total is off\n"); std::abort(); }
        for (int64_t j = 0; j < m; ++j) {
            const double t = (((double)j + 0.5) / (double)m) * total;
            double run = 0.0; int64_t r = 0;
            for (; r < n; ++r) { run += (double)w[(size_t)r]; if (run > t) break; }
            if (a[(size_t)j] != r || got[(size_t)j] != x[(size_t)r]) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)j); std::abort(); }
        }
        OK(fmhip_vec_release(vw)); OK(fmhip_vec_release(vx)); OK(fmhip_vec_release(vu));
        std::printf("cycle %d: resample absent done\n", cycle);
        std::fflush(stdout);
    });
}
