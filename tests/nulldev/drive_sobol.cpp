// drive_sobol.cpp — drives fmhip_bm_generate_sobol_device through the C-ABI on the TEST-ONLY null device under the sanitizers, as
// drive_mersenne.cpp does for the Mersenne-Twister generator: whole processes and blocks behind a path offset (one engine; FMNULL_DEVICES=N:
// a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread), downloaded and compared with
// fmhip_sobol_increments_host narrowed to fp32.  The stand-in (null_sobol.cpp) walks the plan, the direction words and the shifts the engine
// uploaded, so what is checked is the engine: the plan and its slots, the layout of the upload, the workgroup range of a block, the slab;
// then the argument errors.  Twice, with a shutdown and a re-initialisation in between.
#include <atomic>
#include <cmath>
#include <thread>

#include "drive_common.hpp"

namespace fm { extern std::atomic<int> g_null_sobol_launches, g_null_sobol_slots, g_null_sobol_blocks; }

static void block(int32_t seed, int randomize, int construction, const std::vector<double>& dt, int factors, int64_t n, int64_t offset) {
    const int steps = (int)dt.size();
    std::vector<fmhip_vec> h((size_t)steps * factors, 0);
    OK(fmhip_bm_generate_sobol_device(seed, randomize, construction, steps, factors, n, offset, dt.data(), h.data()));
    std::vector<double> want(h.size() * (size_t)n + 1);
    OK(fmhip_sobol_increments_host(seed, randomize, construction, steps, factors, n, offset, dt.data(), want.data()));
    std::vector<float> got((size_t)n + 1);
    for (size_t k = 0; k < h.size(); ++k) {
        int64_t size = -1;
        OK(fmhip_vec_size(h[k], &size));
        if (size != n) { std::fprintf(stderr, "vector %zu has %lld elements, expected %lld\n", k, (long long)size, (long long)n); std::abort(); }
        if (n > 0) OK(fmhip_vec_read_float(h[k], got.data(), n));
        for (int64_t p = 0; p < n; ++p) {
            const float w = (float)want[k * (size_t)n + (size_t)p];
            if (std::memcmp(&w, &got[(size_t)p], 4) != 0) { std::fprintf(stderr, "seed %d construction %d vector %zu path %lld (+%lld): %a, expected %a\n", seed, construction, k, (long long)p, (long long)offset, got[(size_t)p], w); std::abort(); }
        }
        OK(fmhip_vec_release(h[k]));
    }
}

static void scenario(bool thread_engines, bool single_engine) {
    const std::vector<double> dt = { 0.25, 0.0125, 1.5, 0.25, 0.5, 0.125, 2.0 };
    std::thread churn([] {
        for (int i = 0; i < 200; ++i) { fmhip_vec v = 0; OK(fmhip_vec_create_filled(100 + i, 1.0, &v)); OK(fmhip_vec_release(v)); }
    });
    for (int construction = 0; construction < 2; ++construction) {
        const int before = fm::g_null_sobol_launches;
        block(31415, 1, construction, dt, 3, 1000, 0);
        if (single_engine && (fm::g_null_sobol_launches != before + 1 || fm::g_null_sobol_slots != (construction ? 5 : 0) || fm::g_null_sobol_blocks != 4)) {   // 7 steps: depth 3; indices 1 … 1000
            std::fprintf(stderr, "%d launches, %d slots, %d workgroups\n", fm::g_null_sobol_launches - before, fm::g_null_sobol_slots.load(), fm::g_null_sobol_blocks.load()); std::abort();
        }
        block(-7, 0, construction, dt, 3, 1, 0);
        block(31415, 1, construction, dt, 3, 0, 12);
        block(31415, 1, construction, dt, 3, 333, 255);
        block(31415, 1, construction, dt, 3, 5, 777777);
        block(5, 1, construction, { 0.5 }, 1, 300, 0);                                // one step: the terminal value alone
        block(5, 0, construction, { 0.5, 0.25 }, 2, 257, 12345);
        block(9, 1, construction, std::vector<double>(200, 0.05), 5, 40, (int64_t(1) << 30) - 41);      // 1000 dimensions, the end of the sequence
        block(9, 1, construction, std::vector<double>(1024, 0.01), 1, 3, 0);          // the deepest bridge
    }
    if (thread_engines) { std::thread other([&] { block(99, 1, 1, dt, 2, 777, 5); }); other.join(); }
    churn.join();

    fmhip_vec out[21];
    std::vector<double> host(21 * 10);
    const double nan = std::nan(""), inf = HUGE_VAL;
    auto both = [&](int randomize, int construction, int steps, int factors, int64_t n, int64_t offset, const double* steps_dt) {
        EXPECT(fmhip_bm_generate_sobol_device(1, randomize, construction, steps, factors, n, offset, steps_dt, out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_sobol_increments_host(1, randomize, construction, steps, factors, n < 0 ? n : 1, offset, steps_dt, host.data()), FMHIP_ERR_INVALID_ARGUMENT);
    };
    both(1, 1, 0, 3, 10, 0, dt.data()); both(1, 1, 7, 0, 10, 0, dt.data()); both(1, 1, 7, 3, -1, 0, dt.data()); both(1, 1, 7, 3, 10, -1, dt.data());
    both(2, 1, 7, 3, 10, 0, dt.data()); both(-1, 1, 7, 3, 10, 0, dt.data()); both(1, 2, 7, 3, 10, 0, dt.data()); both(1, -1, 7, 3, 10, 0, dt.data());
    both(1, 1, 7, 3, 10, 0, nullptr); both(1, 1, 7, 147, 10, 0, dt.data()); both(1, 1, 7, 3, 10, int64_t(1) << 30, dt.data());
    for (double bad : { -0.5, nan, inf, 0.0 })
        for (int construction = 0; construction < 2; ++construction) {
            if (bad == 0.0 && construction == 0) continue;                             // a zero step is fine increment by increment
            std::vector<double> d = dt; d[4] = bad;
            both(1, construction, 7, 3, 10, 0, d.data());
        }
    EXPECT(fmhip_bm_generate_sobol_device(1, 1, 1, 7, 3, 10, (int64_t(1) << 30) - 10, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_sobol_device(1, 1, 1, 7, 3, 10, 0, dt.data(), nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    std::vector<double> u(1025 * 2);
    EXPECT(fmhip_sobol_points_host(1025, 1, 1, 0, 0, u.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sobol_points_host(0, 1, 1, 0, 0, u.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sobol_points_host(2, int64_t(1) << 30, 1, 0, 0, u.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sobol_points_host(2, 1, 1, 0, 2, u.data()), FMHIP_ERR_INVALID_ARGUMENT);
    OK(fmhip_sobol_points_host(1024, (int64_t(1) << 30) - 2, 2, 7, 1, u.data()));
    std::printf("sobol done\n");
}

int main() { return two_rounds([](int, bool thread_engines, bool single_engine) { scenario(thread_engines, single_engine); }); }
