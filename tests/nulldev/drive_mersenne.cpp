// drive_mersenne.cpp — drives fmhip_bm_generate_mersenne_device through the C-ABI on the TEST-ONLY null device under the sanitizers: whole
// motions and blocks behind a path offset (one engine; FMNULL_DEVICES=N: behind a device list of N shards, every shard its own block;
// FMNULL_THREAD_ENGINES=1: an engine per caller thread), downloaded and compared with fmhip_mersenne_increments narrowed to fp32 — the
// stand-in launchers (null_mt.cpp) generate with the host code from the state the engine hands them, so what is checked is the engine:
// seeding, distances, the layout of the slab, the handles; then the errors that are found on the host, with another thread creating and
// releasing vectors meanwhile.  Twice, with a shutdown and a re-initialisation in between.
#include <thread>

#include "drive_common.hpp"

static void block(int32_t seed, const std::vector<double>& dt, int factors, int64_t n, int64_t offset) {
    const int steps = (int)dt.size();
    compare_block(seed, (size_t)steps * factors, n, offset,
                  [&](fmhip_vec* h) { return fmhip_bm_generate_mersenne_device(seed, steps, factors, n, offset, dt.data(), h); },
                  [&](double* host) { return fmhip_mersenne_increments(seed, steps, factors, offset + n, dt.data(), host); });
}

static void scenario(bool thread_engines) {
    const std::vector<double> dt = { 0.25, 0.0, 1.5 };
    std::thread churn([] {                                  // another caller of the same process meanwhile
        for (int i = 0; i < 200; ++i) { fmhip_vec v = 0; OK(fmhip_vec_create_filled(100 + i, 1.0, &v)); OK(fmhip_vec_release(v)); }
    });
    block(31415, dt, 2, 1000, 0);
    block(-7, dt, 2, 1, 0);
    block(31415, dt, 2, 0, 12);
    block(31415, dt, 2, 333, 1);                            // an odd offset
    block(31415, dt, 2, 5, 20001);                          // 120 006 words in front: several table rows
    block(1, { 1.0 }, 1, 4097, 3);
    if (thread_engines) { std::thread other([&] { block(99, dt, 1, 777, 5); }); other.join(); }
    churn.join();
    fmhip_vec out[6];
    const double bad[3] = { 0.25, -1.0, 1.5 };
    EXPECT(fmhip_bm_generate_mersenne_device(1, 0, 2, 10, 0, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 0, 10, 0, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, -1, 0, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, 10, -1, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, 10, 0, nullptr, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, 10, 0, dt.data(), nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, 10, 0, bad, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_bm_generate_mersenne_device(1, 3, 2, 10, (int64_t(1) << 44) / 12, dt.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    std::printf("mersenne done\n");
}

int main() { return two_rounds([](int, bool thread_engines, bool) { scenario(thread_engines); }); }
