// drive_binned.cpp — drives fmhip_binned_cross_moments and fmhip_binned_evaluate through the C-ABI on the TEST-ONLY null device under the
// sanitizers: vectors uploaded from the host (small integers: every sum is exact in fp64, so shards may add in any order), stored and
// pending operands, the constant 1, 1 / 2 / 16 / 64 bins, all (n_x, n_y) shapes, with another thread releasing the INPUTS of pending
// operands while the call runs; counts, sums and the estimate are compared with fmhip_binned_*_host bit for bit.  Then the errors that are
// found on the host.  Twice, with a shutdown and a re-initialisation in between.  FMNULL_DEVICES=N: behind a device list of N shards;
// FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked about by a thread that does not own them.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_binned_evaluate in which the allocation of the output fails.
// The null device computes nothing element-wise, so pending operands are only counted on (their values are whatever the buffers hold).
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V upload(const std::vector<float>& v) { V h = 0; OK(fmhip_vec_create_from_float(v.data(), (int64_t)v.size(), &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

struct Data { std::vector<float> key; std::vector<std::vector<float>> col; V hkey; std::vector<V> hcol; };

static void compare(const Data& d, const std::vector<double>& bounds, const std::vector<int>& xi, const std::vector<int>& yi) {
    const int n_bins = (int)bounds.size() + 1, nx = (int)xi.size(), ny = (int)yi.size(), q = nx * (nx + 1) / 2 + nx * ny;
    std::vector<V> hx, hy; std::vector<const float*> px, py;
    for (int i : xi) { hx.push_back(i < 0 ? 0 : d.hcol[(size_t)i]); px.push_back(i < 0 ? nullptr : d.col[(size_t)i].data()); }
    for (int i : yi) { hy.push_back(d.hcol[(size_t)i]); py.push_back(d.col[(size_t)i].data()); }
    std::vector<int64_t> counts((size_t)n_bins, -1), want_counts((size_t)n_bins, -2);
    std::vector<double> sums((size_t)n_bins * q, -1.0), want_sums((size_t)n_bins * q, -2.0);
    const double* b = bounds.empty() ? nullptr : bounds.data();
    OK(fmhip_binned_cross_moments(d.hkey, b, n_bins, hx.data(), nx, ny ? hy.data() : nullptr, ny, counts.data(), sums.data()));
    OK(fmhip_binned_cross_moments_host(d.key.data(), (int64_t)d.key.size(), b, n_bins, px.data(), nx, ny ? py.data() : nullptr, ny, want_counts.data(), want_sums.data()));
    if (counts != want_counts || std::memcmp(sums.data(), want_sums.data(), sums.size() * 8) != 0) { std::fprintf(stderr, "binned moments differ from the definition (%d bins, %d x, %d y)\n", n_bins, nx, ny); std::abort(); }
    // the estimate: coefficients that are small integers, a new vector
    std::vector<double> coef((size_t)n_bins * nx);
    for (size_t i = 0; i < coef.size(); ++i) coef[i] = (double)((int)(i % 5) - 2);
    V est = 0;
    OK(fmhip_binned_evaluate(d.hkey, b, n_bins, hx.data(), nx, coef.data(), &est));
    std::vector<float> got(d.key.size()), want(d.key.size());
    OK(fmhip_vec_read_float(est, got.data(), (int64_t)got.size()));
    OK(fmhip_binned_evaluate_host(d.key.data(), (int64_t)d.key.size(), b, n_bins, px.data(), nx, coef.data(), want.data()));
    if (std::memcmp(got.data(), want.data(), got.size() * 4) != 0) { std::fprintf(stderr, "binned estimate differs from the definition (%d bins, %d x)\n", n_bins, nx); std::abort(); }
    rel(est);
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const size_t n = 2051;
    Data d;
    d.key.resize(n); d.col.assign(5, std::vector<float>(n));
    for (size_t p = 0; p < n; ++p) {
        d.key[p] = (float)((int)((p * 37) % 101) - 50);
        for (size_t c = 0; c < 5; ++c) d.col[c][p] = (float)((int)((p * (c + 3)) % 17) - 8);
    }
    d.key[5] = std::numeric_limits<float>::quiet_NaN(); d.key[6] = std::numeric_limits<float>::infinity(); d.key[7] = -std::numeric_limits<float>::infinity();
    d.key[8] = -0.0f; d.key[9] = 0.0f;
    d.hkey = upload(d.key);
    for (const auto& c : d.col) d.hcol.push_back(upload(c));
    std::vector<double> b16, b64;
    for (int j = 1; j < 16; ++j) b16.push_back(-50.0 + 6.25 * j);
    for (int j = 1; j < 64; ++j) b64.push_back(j == 1 ? -std::numeric_limits<double>::infinity() : j == 63 ? std::numeric_limits<double>::infinity() : -52.0 + 1.7 * j);
    auto all = [&] {
        compare(d, {}, { -1, 0 }, { 1 });
        compare(d, { 0.0 }, { -1, 0 }, { 1 });
        compare(d, b16, { -1, 0 }, { 1 });
        compare(d, b16, { 0 }, {});
        compare(d, b16, { -1 }, {});
        compare(d, b64, { -1, 0, 2 }, { 1, 3, 4, 0 });          // 18 products: four bins per slice, sixteen slices
        compare(d, b64, { 0, -1, -1 }, { 1 });
        compare(d, { 1.0, 1.0, 1.0, 2.0 }, { 2, 0 }, { 1, 1 }); // equal bounds: empty bins; the same vector twice
    };
    if (thread_engines) { std::thread asker(all); asker.join(); }      // vectors of another thread's engine
    all();
    // pending operands whose INPUTS are released by another thread during the calls: only the calls' own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, dv = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, d.hcol[0], 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &dv));
        inputs.push_back(in); derived.push_back(dv);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, d.hcol[1], (double)i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    {
        std::vector<int64_t> counts(16); std::vector<double> sums(16 * 18); V est = 0;
        const V x[3] = { 0, derived[0], derived[1] }, y[4] = { derived[2], derived[3], derived[4], d.hcol[2] };
        OK(fmhip_binned_cross_moments(derived[5], b16.data(), 16, x, 3, y, 4, counts.data(), sums.data()));
        std::vector<double> coef(16 * 3, 0.5);
        OK(fmhip_binned_evaluate(derived[5], b16.data(), 16, x, 3, coef.data(), &est));
        int64_t size = 0; OK(fmhip_vec_size(est, &size));
        if (size != (int64_t)n) { std::fprintf(stderr, "the estimate has %lld elements\n", (long long)size); std::abort(); }
        rel(est);
    }
    releaser.join();
    // found on the host, before any launch
    int64_t counts[64]; double out[64 * 18]; V est = 0;
    const V k = d.hkey, x2[2] = { 0, d.hcol[0] }, four[4] = { d.hcol[0], d.hcol[0], d.hcol[0], d.hcol[0] }, five[5] = { k, k, k, k, k }, zero_y[1] = { 0 };
    const double nan_b[2] = { 0.0, std::nan("") }, unsorted[2] = { 1.0, 0.5 }, fine[2] = { 0.0, 1.0 }, coef[6] = { 0 };
    std::vector<double> b65(65, 0.0);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 0, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, four, 4, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, five, 5, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, five, -1, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 0, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, b65.data(), 65, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, nullptr, 3, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, nullptr, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, nullptr, 1, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, nullptr, 0, nullptr, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, nullptr, 0, counts, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, unsorted, 3, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, nan_b, 3, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, zero_y, 1, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(0, fine, 3, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_cross_moments(k + 1000000, fine, 3, x2, 2, nullptr, 0, counts, out), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_binned_evaluate(k, fine, 3, x2, 2, nullptr, &est), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_evaluate(k, fine, 3, x2, 2, coef, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_evaluate(k, unsorted, 3, x2, 2, coef, &est), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_evaluate(0, fine, 3, x2, 2, coef, &est), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_binned_evaluate(k, fine, 3, four, 4, coef, &est), FMHIP_ERR_INVALID_ARGUMENT);
    V shorter = 0; OK(fmhip_vec_create_filled((int64_t)n - 1, 1.0, &shorter));
    const V mixed[2] = { 0, shorter };
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, mixed, 2, nullptr, 0, counts, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_binned_cross_moments(k, fine, 3, x2, 2, &shorter, 1, counts, out), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_binned_evaluate(k, fine, 3, mixed, 2, coef, &est), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_binned_cross_moments(shorter, fine, 3, mixed, 2, nullptr, 0, counts, out), FMHIP_OK);
    rel(shorter);
    for (V v : derived) rel(v);
    rel(d.hkey); for (V v : d.hcol) rel(v);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the output of one fmhip_binned_evaluate is its one pool allocation.  Without it this is
// the counting run that says where it is.
static int failure() {
    OK(fmhip_init(0));
    const size_t n = 2051;
    std::vector<float> key(n), col(n), want(n), got(n);
    for (size_t p = 0; p < n; ++p) { key[p] = (float)((int)((p * 37) % 101) - 50); col[p] = (float)((int)((p * 3) % 17) - 8); }
    const V hkey = upload(key), x[2] = { 0, upload(col) };
    const float* px[2] = { nullptr, col.data() };
    const double bounds[3] = { -20.0, 0.0, 20.0 }, coef[8] = { 1.0, 2.0, -1.0, 0.0, 3.0, -2.0, 0.0, 1.0 };
    OK(fmhip_binned_evaluate_host(key.data(), (int64_t)n, bounds, 4, px, 2, coef, want.data()));
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V est = 0;
        const int st = fmhip_binned_evaluate(hkey, bounds, 4, x, 2, coef, &est);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            OK(fmhip_vec_read_float(est, got.data(), (int64_t)n));
            if (std::memcmp(got.data(), want.data(), n * 4) != 0) { std::fprintf(stderr, "attempt %d: the estimate differs from the definition\n", attempt); std::abort(); }
            rel(est);
        } else if (est != 0) { std::fprintf(stderr, "a failed call wrote its output\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) {
            std::fprintf(stderr, "a binned_evaluate left %lld vectors and %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use));
            std::abort();
        }
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(hkey); rel(x[1]);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: binned done\n", cycle);
        std::fflush(stdout);
    });
}
