// drive_select_absent.cpp — a build of the engine WITHOUT the launchers of select_kernel.hip (no stand-in for them is linked: the weak
// references stay null) on the TEST-ONLY null device: fmhip_compress, fmhip_expand and fmhip_gather answer FMHIP_ERR_UNSUPPORTED — after
// their argument checks, which still come first — and never fall back; the definitions (the _host twins) need no kernel; nothing is left
// behind.
#include "drive_common.hpp"

int main() {
    return two_rounds([](int cycle, bool, bool) {
        const int64_t n = 1000;
        std::vector<float> m((size_t)n), x((size_t)n);
        for (int64_t p = 0; p < n; ++p) { m[(size_t)p] = (float)((p * 37) % 101) - 50.f; x[(size_t)p] = (float)p; }
        fmhip_vec vm = 0, vx = 0, longer = 0, out = 0, positions = 0;
        OK(fmhip_vec_create_from_float(m.data(), n, &vm));
        OK(fmhip_vec_create_from_float(x.data(), n, &vx));
        OK(fmhip_vec_create_from_float(x.data(), n - 1, &longer));
        fmhip_pool_stats_t before, after;
        OK(fmhip_pool_stats(&before));
        int64_t count = -7;
        EXPECT(fmhip_compress(vm, &vx, 9, &out, &positions, &count), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_compress(vm, &longer, 1, &out, &positions, &count), FMHIP_ERR_SIZE_MISMATCH);
        EXPECT(fmhip_expand(vm, &vx, 0, 0.0, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_gather(0, &vx, 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_compress(vm, &vx, 1, &out, &positions, &count), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_compress(vm, nullptr, 0, nullptr, nullptr, &count), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_expand(vm, &vx, 1, 0.0, &out), FMHIP_ERR_UNSUPPORTED);
        EXPECT(fmhip_gather(vm, &vx, 1, &out), FMHIP_ERR_UNSUPPORTED);
        if (out != 0 || positions != 0 || count != -7) { std::fprintf(stderr, "a refused call wrote its outputs\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call left %lld vectors, %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use)); std::abort(); }
        // the definitions need no kernel
        std::vector<float> got((size_t)n), back((size_t)n), again((size_t)n);
        std::vector<int64_t> pos((size_t)n, -7);
        const float* in[1] = { x.data() }; float* columns[1] = { got.data() };
        OK(fmhip_compress_host(m.data(), n, in, 1, columns, pos.data(), &count));
        int64_t q = 0;
        for (int64_t p = 0; p < n; ++p) if (m[(size_t)p] >= 0.f) { if (pos[(size_t)q] != p || got[(size_t)q] != x[(size_t)p]) { std::fprintf(stderr, "the definition is off at %lld\n", (long long)p); std::abort(); } ++q; }
        if (q != count) { std::fprintf(stderr, "the count is off\n"); std::abort(); }
        const float* sin[1] = { got.data() }; float* bout[1] = { back.data() };
        OK(fmhip_expand_host(m.data(), n, sin, 1, count, -1.0, bout));
        EXPECT(fmhip_expand_host(m.data(), n, sin, 1, count - 1, -1.0, bout), FMHIP_ERR_SIZE_MISMATCH);
        for (int64_t p = 0; p < n; ++p) if (back[(size_t)p] != (m[(size_t)p] >= 0.f ? x[(size_t)p] : -1.f)) { std::fprintf(stderr, "the expansion is off at %lld\n", (long long)p); std::abort(); }
        float* gout[1] = { again.data() };
        OK(fmhip_gather_host(x.data(), n, in, 1, n, gout));                       // x[p] = p: the identity
        if (std::memcmp(again.data(), x.data(), (size_t)n * 4) != 0) { std::fprintf(stderr, "the gather is off\n"); std::abort(); }
        OK(fmhip_vec_release(vm)); OK(fmhip_vec_release(vx)); OK(fmhip_vec_release(longer));
        std::printf("cycle %d: select absent done\n", cycle);
        std::fflush(stdout);
    });
}
