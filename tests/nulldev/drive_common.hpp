// drive_common.hpp — what the drivers of the TEST-ONLY null device share: the status macros, the two rounds of initialisation and shutdown,
// and the comparison of a generated block with its host definition.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fmhip.h"

#define OK(x) do { const int st_ = (x); if (st_ != FMHIP_OK) { std::fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, st_, fmhip_last_error()); std::abort(); } } while (0)
#define EXPECT(x, code) do { const int st_ = (x); if (st_ != (code)) { std::fprintf(stderr, "%s:%d: %s -> %d, expected %d (%s)\n", __FILE__, __LINE__, #x, st_, (int)(code), fmhip_last_error()); std::abort(); } } while (0)

// main(): scenario(round, thread_engines, single_engine) twice, with a shutdown and a re-initialisation in between.  FMNULL_DEVICES=N: behind
// a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread; neither: one engine (single_engine).
template <class Scenario>
int two_rounds(Scenario scenario) {
    for (int round = 0; round < 2; ++round) {
        const int n_devices = std::getenv("FMNULL_DEVICES") ? std::atoi(std::getenv("FMNULL_DEVICES")) : 1;
        const bool thread_engines = n_devices <= 1 && std::getenv("FMNULL_THREAD_ENGINES");
        if (n_devices > 1) { std::vector<int> devices((size_t)n_devices, 0); OK(fmhip_init_devices(devices.data(), n_devices)); }
        else OK(fmhip_init(0));
        if (thread_engines) OK(fmhip_set_thread_engines(1, nullptr));
        scenario(round, thread_engines, n_devices <= 1 && !thread_engines);
        OK(fmhip_shutdown());
    }
    return 0;
}

// A block of `count` vectors of n paths behind `offset`: device(handles) generates it, host(doubles) is the definition of the offset + n
// paths from the start of the stream; every float is downloaded and compared with the definition narrowed to fp32, bit for bit.
template <class Device, class Host>
void compare_block(int32_t seed, size_t count, int64_t n, int64_t offset, Device device, Host host) {
    std::vector<fmhip_vec> h(count, 0);
    OK(device(h.data()));
    std::vector<double> want_all(count * (size_t)(offset + n));
    OK(host(want_all.data()));
    std::vector<float> got((size_t)n + 1);
    for (size_t k = 0; k < count; ++k) {
        int64_t size = -1;
        OK(fmhip_vec_size(h[k], &size));
        if (size != n) { std::fprintf(stderr, "vector %zu has %lld elements, expected %lld\n", k, (long long)size, (long long)n); std::abort(); }
        if (n > 0) OK(fmhip_vec_read_float(h[k], got.data(), n));
        for (int64_t p = 0; p < n; ++p) {
            const float want = (float)want_all[k * (size_t)(offset + n) + (size_t)(offset + p)];
            if (std::memcmp(&want, &got[(size_t)p], 4) != 0) { std::fprintf(stderr, "seed %d vector %zu path %lld (+%lld): %a, expected %a\n", seed, k, (long long)p, (long long)offset, got[(size_t)p], want); std::abort(); }
        }
        OK(fmhip_vec_release(h[k]));
    }
}
