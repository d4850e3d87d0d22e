// drive_kreg.cpp — drives fmhip_kernel_moments through the C-ABI on the TEST-ONLY null device under the sanitizers: vectors uploaded from the
// host (dyadic keys k/8, points on multiples of 1/4, bandwidths 0.5 / 1 / 2, small integer y: every term and every sum is exact in fp64, so
// shards may add in any order), stored and pending operands, 1 / 2 / 36 / 37 / 256 points, every (order, n_y) shape and every kernel, with
// another thread releasing the INPUTS of pending operands while the call runs; the sums are compared with fmhip_kernel_moments_host bit for
// bit.  Then the errors that are found on the host, with nothing allocated.  Twice, with a shutdown and a re-initialisation in between.
// FMNULL_DEVICES=N: behind a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked about by a
// thread that does not own them.  The null device computes nothing element-wise, so pending operands are only counted on.
#include <cmath>
#include <limits>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V upload(const std::vector<float>& v) { V h = 0; OK(fmhip_vec_create_from_float(v.data(), (int64_t)v.size(), &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

struct Data { std::vector<float> key; std::vector<std::vector<float>> col; V hkey; std::vector<V> hcol; };

static void compare(const Data& d, const std::vector<double>& points, const std::vector<double>& h, int kernel, int order, const std::vector<int>& yi) {
    const int Q = (int)points.size(), ny = (int)yi.size(), qe = order == 0 ? 1 + ny : 3 + 2 * ny;
    std::vector<V> hy; std::vector<const float*> py;
    for (int i : yi) { hy.push_back(d.hcol[(size_t)i]); py.push_back(d.col[(size_t)i].data()); }
    std::vector<double> sums((size_t)Q * qe, -1.0), want((size_t)Q * qe, -2.0);
    OK(fmhip_kernel_moments(d.hkey, points.data(), h.data(), Q, kernel, order, ny ? hy.data() : nullptr, ny, sums.data()));
    OK(fmhip_kernel_moments_host(d.key.data(), (int64_t)d.key.size(), points.data(), h.data(), Q, kernel, order, ny ? py.data() : nullptr, ny, want.data()));
    if (std::memcmp(sums.data(), want.data(), sums.size() * 8) != 0) { std::fprintf(stderr, "kernel moments differ from the definition (%d points, kernel %d, order %d, %d y)\n", Q, kernel, order, ny); std::abort(); }
}

static std::vector<double> grid(int Q, double from, double step) { std::vector<double> p((size_t)Q); for (int q = 0; q < Q; ++q) p[(size_t)q] = from + step * (q / 2 * 2); return p; }      // every point twice

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const size_t n = 2051;
    Data d;
    d.key.resize(n); d.col.assign(5, std::vector<float>(n));
    for (size_t p = 0; p < n; ++p) {
        d.key[p] = (float)((int)((p * 37) % 523) - 261) * 0.125f;                      // k/8 in [-32.7, 32.7]
        for (size_t c = 0; c < 5; ++c) d.col[c][p] = (float)((int)((p * (c + 3)) % 33) - 16);
    }
    d.key[5] = std::numeric_limits<float>::quiet_NaN(); d.key[6] = std::numeric_limits<float>::infinity(); d.key[7] = -std::numeric_limits<float>::infinity();
    d.key[8] = -0.0f; d.key[9] = 0.0f;
    d.hkey = upload(d.key);
    for (const auto& c : d.col) d.hcol.push_back(upload(c));
    auto all = [&] {
        for (int kernel = FMHIP_KERNEL_UNIFORM; kernel <= FMHIP_KERNEL_TRIWEIGHT; ++kernel) {
            compare(d, { 0.25 }, { 2.0 }, kernel, 0, {});
            compare(d, { -1.0, 1.5 }, { 0.5, 1.0 }, kernel, 1, { 1 });
        }
        for (int Q : { 36, 37, 256 }) {
            const std::vector<double> p = grid(Q, -32.0, 0.25), h1((size_t)Q, 1.0), h2((size_t)Q, 2.0);
            compare(d, p, h1, FMHIP_KERNEL_EPANECHNIKOV, 0, { 0 });                     // 2 entries per point: 36 is one slice, 37 two
            compare(d, p, h2, FMHIP_KERNEL_QUARTIC, 1, { 0, 1, 2, 3 });                 // 11 entries per point: 6 points per slice
            compare(d, p, h1, FMHIP_KERNEL_TRIANGULAR, 0, { 4, 4, 0, 1 });              // the same vector twice
            compare(d, p, h2, FMHIP_KERNEL_UNIFORM, 1, {});
        }
        std::vector<double> p = grid(64, -8.0, 0.25), h(64);
        for (int q = 0; q < 64; ++q) h[(size_t)q] = q < 20 ? 2.0 : q < 40 ? 1.0 : 2.0;   // bandwidths per point; lower and upper stay monotone
        for (int q = 0; q < 64; ++q) p[(size_t)q] = -8.0 + 0.25 * q + (q >= 20 ? 1.0 : 0.0) + (q >= 40 ? 1.0 : 0.0);
        compare(d, p, h, FMHIP_KERNEL_TRIWEIGHT, 1, { 2 });
    };
    if (thread_engines) { std::thread asker(all); asker.join(); }      // vectors of another thread's engine
    all();
    // pending operands whose INPUTS are released by another thread during the call: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 5; ++i) {
        V in = 0, dv = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, d.hcol[0], 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &dv));
        inputs.push_back(in); derived.push_back(dv);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, d.hcol[1], (double)i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    {
        const std::vector<double> p = grid(40, -4.0, 0.25), h(40, 1.0);
        std::vector<double> sums(40 * 11);
        const V y[4] = { derived[1], derived[2], derived[3], d.hcol[2] };
        OK(fmhip_kernel_moments(derived[0], p.data(), h.data(), 40, FMHIP_KERNEL_EPANECHNIKOV, 1, y, 4, sums.data()));
    }
    releaser.join();
    // found on the host, before any flush or launch: nothing is allocated, nothing pending is computed
    V pending = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, d.hcol[0], 7.0, &pending));
    fmhip_pool_stats_t before, after;
    OK(fmhip_pool_stats(&before));
    double out[257 * 11];
    const V k = d.hkey, five[5] = { k, k, k, k, k }, zero_y[1] = { 0 }, one_y[1] = { pending };
    const double fine[3] = { 0.0, 1.0, 2.0 }, h3[3] = { 1.0, 1.0, 1.0 }, unsorted[3] = { 0.0, 2.0, 1.0 }, nan_p[3] = { 0.0, std::nan(""), 2.0 }, inf_p[3] = { 0.0, 1.0, std::numeric_limits<double>::infinity() };
    const double zero_h[3] = { 1.0, 0.0, 1.0 }, neg_h[3] = { 1.0, -1.0, 1.0 }, nan_h[3] = { 1.0, std::nan(""), 1.0 }, lower_down[3] = { 1.0, 2.5, 2.5 }, upper_down[3] = { 2.5, 1.0, 1.0 };
    std::vector<double> p257(257, 0.0), h257(257, 1.0);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 0, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, p257.data(), h257.data(), 257, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, five, 5, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, five, -1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 2, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, -1, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, 5, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, -1, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, nullptr, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, nullptr, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, unsorted, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, nan_p, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, inf_p, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, zero_h, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, neg_h, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, nan_h, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(k, fine, lower_down, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);      // lower: -1, -1.5
    EXPECT(fmhip_kernel_moments(k, fine, upper_down, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);      // upper: 2.5, 2
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, zero_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments(0, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, one_y, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    OK(fmhip_pool_stats(&after));
    if (after.n_kernel_launches != before.n_kernel_launches || after.bytes_in_use != before.bytes_in_use) { std::fprintf(stderr, "a refused call flushed or allocated\n"); std::abort(); }
    EXPECT(fmhip_kernel_moments(k + 1000000, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 0, out), FMHIP_ERR_INVALID_HANDLE);
    V shorter = 0; OK(fmhip_vec_create_filled((int64_t)n - 1, 1.0, &shorter));
    EXPECT(fmhip_kernel_moments(k, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, &shorter, 1, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_kernel_moments(shorter, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 0, out), FMHIP_OK);
    const float one[1] = { 1.0f };
    EXPECT(fmhip_kernel_moments_host(nullptr, 1, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments_host(one, 0, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_kernel_moments_host(one, 1, fine, h3, 3, FMHIP_KERNEL_UNIFORM, 0, nullptr, 0, out), FMHIP_OK);
    rel(shorter); rel(pending);
    for (V v : derived) rel(v);
    rel(d.hkey); for (V v : d.hcol) rel(v);
}

int main() {
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: kreg done\n", cycle);
        std::fflush(stdout);
    });
}
