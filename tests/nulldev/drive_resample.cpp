// drive_resample.cpp — drives fmhip_resample through the C-ABI on the TEST-ONLY null device under the sanitizers.  The vectors hold real
// data and the stand-in of null_resample.cpp walks the chunks and the tiles the kernels' way, so results are CHECKED against the
// definition (fmhip_resample_host): every scheme and equal weights, 0, 1 and 8 companions, with and without ancestors and total, at n = 1,
// 65, one tile + 1, the smallest n with three chunks and 300 007 (scratch, temporary and stage grow between the calls), m below, at and
// above n, and 65 and 1 again behind the large one; degenerate totals; NaN, negative and out-of-range uniforms.  Pending operands, every
// argument error that is found on the host.  Twice, with a shutdown and a re-initialisation in between; then once more behind a device
// list of ONE shard.  FMNULL_DEVICES=N: behind N shards every call is FMHIP_ERR_UNSUPPORTED and leaves nothing behind;
// FMNULL_THREAD_ENGINES=1: the calls come from a thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one weighted fmhip_resample in which a pool allocation fails — an output or
// the temporary of P.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"
#include "../../finmath-lib-cuda-extensions_amd/csrc/resample_host.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// kind 0: weights over sixteen decades with zeros, a NaN, a negative and a -0.0 among them; kind 1: values with a NaN payload and a -0.0
static F data(int64_t n, uint32_t seed, int kind) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (p % 5 == 2) x = 0.f;
        if (kind == 0) { if (p % 11 == 3) x = -x; if (p % 97 == 50) x = std::numeric_limits<float>::quiet_NaN(); if (p % 13 == 7) x = -0.f; }
        else { if (p % 7 == 1) { const uint32_t bits = 0x7fc01234u + (uint32_t)(p & 0xff); std::memcpy(&x, &bits, 4); } if (p % 7 == 3) x = -0.f; }
        a[(size_t)p] = x;
    }
    if (kind == 0 && n == 1) a[0] = 3.f;
    return a;
}
static F uniforms(int64_t m, uint32_t seed) {
    F u((size_t)m);
    uint32_t s = seed * 747796405u + 2891336453u;
    for (int64_t j = 0; j < m; ++j) { s = s * 1664525u + 1013904223u; u[(size_t)j] = (float)(s >> 8) * (1.0f / 16777216.0f); }
    if (m > 4) { u[1] = std::numeric_limits<float>::quiet_NaN(); u[2] = -0.5f; u[3] = 1.0f; u[4] = std::nextafter(1.0f, 0.0f); }
    return u;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static int64_t live() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st.n_live_vectors; }

// one call against the definition; vw == 0: equal weights
static void check(V vw, const F* w, const std::vector<V>& vx, const std::vector<F>& x, int64_t n, int scheme, int64_t m, double offset, V vu, const F& u, bool want_ancestors, bool want_total) {
    const int k = (int)vx.size();
    std::vector<F> want((size_t)k, F((size_t)m));
    std::vector<int64_t> a((size_t)m, -7);
    const float* in[8]; float* columns[8];
    for (int i = 0; i < k; ++i) { in[i] = x[(size_t)i].data(); columns[i] = want[(size_t)i].data(); }
    double total_host = -1.0, total = -1.0;
    const bool anc = want_ancestors || k == 0;
    OK(fmhip_resample_host(w ? w->data() : nullptr, n, scheme, m, offset, scheme ? u.data() : nullptr, in, k, columns, anc ? a.data() : nullptr, &total_host));
    V out[8] = { 0 }, va = 0;
    OK(fmhip_resample(vw, scheme, m, offset, scheme ? vu : 0, vx.data(), k, out, anc ? &va : nullptr, want_total ? &total : nullptr));
    if (want_total && std::memcmp(&total, &total_host, 8) != 0) die("the total", n, m);
    for (int i = 0; i < k; ++i) {
        const F got = download(out[i], m);
        for (int64_t j = 0; j < m; ++j) if (!same(got[(size_t)j], want[(size_t)i][(size_t)j])) die("a gathered vector", n, j);
        rel(out[i]);
    }
    if (anc) {
        const F got = download(va, m);
        for (int64_t j = 0; j < m; ++j) {
            float f = (float)a[(size_t)j];
            if (a[(size_t)j] < 0) std::memcpy(&f, &fm::FM_RESAMPLE_NAN_BITS, 4);
            if (!same(got[(size_t)j], f)) die("the ancestors", n, j);
        }
        rel(va);
    }
}

static void check_all(V vw, const F& w, const std::vector<V>& vx, const std::vector<F>& x, int64_t n) {
    const int64_t ms[3] = { n, std::max<int64_t>(1, n / 4), std::min<int64_t>(4 * n, n + 4099) };
    for (int64_t m : ms) {
        const F u = uniforms(m, (uint32_t)(n + m));
        V vu = upload(u);
        const std::vector<V> one(vx.begin(), vx.begin() + 1), none;
        const std::vector<F> one_x(x.begin(), x.begin() + 1), none_x;
        for (int scheme = 0; scheme < 3; ++scheme) {
            check(vw, &w, one, one_x, n, scheme, m, 0.375, vu, u, scheme == 1, true);
            check(0, nullptr, one, one_x, n, scheme, m, 0.0, vu, u, scheme == 2, scheme == 0);
        }
        check(vw, &w, vx, x, n, 0, m, 0.999999, vu, u, true, false);
        check(vw, &w, none, none_x, n, 2, m, 0.0, vu, u, true, true);
        rel(vu);
    }
    if (std::memcmp(download(vw, n).data(), w.data(), (size_t)n * 4) != 0) die("the weights changed", n, 0);
    if (std::memcmp(download(vx[0], n).data(), x[0].data(), (size_t)n * 4) != 0) die("a value vector changed", n, 0);
}

static void degenerate(int64_t n) {
    F zero((size_t)n, 0.f), inf((size_t)n, 1.f), x = data(n, 3, 1);
    zero[0] = -1.f; inf[(size_t)n / 2] = std::numeric_limits<float>::infinity();
    const F u = uniforms(n, 9);
    V vz = upload(zero), vi = upload(inf), vx = upload(x), vu = upload(u);
    for (int scheme = 0; scheme < 3; ++scheme) {
        check(vz, &zero, { vx }, { x }, n, scheme, n, 0.5, vu, u, true, true);
        check(vi, &inf, { vx }, { x }, n, scheme, n, 0.5, vu, u, true, true);
    }
    rel(vz); rel(vi); rel(vx); rel(vu);
}

static void refusals(V vw, V vx, int64_t n) {
    const int64_t before = live();
    const F u = uniforms(n, 1);
    V vu = upload(u), short_x = upload(F((size_t)n + 1, 1.f));
    V out[9] = { 0 }, anc = 0; double total = -1.0;
    V nine[9] = { vx, vx, vx, vx, vx, vx, vx, vx, vx }, with_zero[2] = { vx, 0 };
    const int S = FMHIP_RESAMPLE_SYSTEMATIC, M = FMHIP_RESAMPLE_MULTINOMIAL;
    EXPECT(fmhip_resample(vw, 3, n, 0.5, vu, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, -1, n, 0.5, vu, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, 0, 0.5, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, int64_t(1) << 31, 0.5, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, nine, 9, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, &vx, -1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, nullptr, 0, nullptr, nullptr, &total), FMHIP_ERR_INVALID_ARGUMENT);      // nothing asked for
    EXPECT(fmhip_resample(0, M, n, 0.0, vu, nullptr, 0, nullptr, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);         // neither weights nor a value vector
    EXPECT(fmhip_resample(vw, S, n, 1.0, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, -0.25, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, std::numeric_limits<double>::quiet_NaN(), 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, M, n, 0.0, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);                  // no uniforms
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, nullptr, 1, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, &vx, 1, nullptr, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, with_zero, 2, out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_resample(vw, S, n, 0.5, 0, &short_x, 1, out, &anc, &total), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_resample(vw, M, n + 1, 0.0, vu, &vx, 1, out, &anc, &total), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_resample(vw + 12345, S, n, 0.5, 0, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_resample(vw, M, n, 0.0, vu + 12345, &vx, 1, out, &anc, &total), FMHIP_ERR_INVALID_HANDLE);
    rel(vu); rel(short_x);
    if (out[0] != 0 || anc != 0 || total != -1.0 || live() != before) die("a refused call left something behind", n, live() - before);
}

static void unsupported(V vw, V vx, int64_t n) {
    const int64_t before = live();
    const F u = uniforms(n, 1);
    V vu = upload(u), out = 0, anc = 0; double total = -1.0;
    EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_SYSTEMATIC, n, 0.5, 0, &vx, 1, &out, &anc, &total), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_resample(0, FMHIP_RESAMPLE_MULTINOMIAL, n, 0.0, vu, &vx, 1, &out, nullptr, &total), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_resample(vw, FMHIP_RESAMPLE_STRATIFIED, n, 0.0, vu, nullptr, 0, nullptr, &anc, nullptr), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_resample(vw, 7, n, 0.5, 0, &vx, 1, &out, &anc, &total), FMHIP_ERR_INVALID_ARGUMENT);               // the checks still come first
    rel(vu);
    if (out != 0 || anc != 0 || total != -1.0 || live() != before) die("a device list of several shards left something behind", n, live() - before);
}

static const int64_t THREE = [] { int64_t n = 2 * fm::prefix_chunk_elems(1) + 1; while (n % 64 == 0) ++n; return n; }();

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    if (fm::prefix_blocks(THREE) != 3 || fm::prefix_blocks(THREE - 1) != 2) die("the smallest n with three chunks", THREE, 0);
    const int64_t sizes[7] = { 1, 65, fm::FM_PREFIX_TILE + 1, THREE, 300007, 65, 1 };
    for (int64_t n : sizes) {
        const F w = data(n, (uint32_t)n, 0);
        std::vector<F> x; std::vector<V> vx;
        for (int i = 0; i < 8; ++i) { x.push_back(data(n, (uint32_t)(n + 1 + i), 1)); vx.push_back(upload(x.back())); }
        V vw = upload(w);
        if (sharded) { unsupported(vw, vx[0], n); }
        else {
            const int64_t before = live();
            if (thread_engines) {
                std::thread asker([&] { check_all(vw, w, vx, x, n); });                  // a thread that owns none of them
                asker.join();
                if (n < 300000) check_all(vw, w, vx, x, n);                              // and the owner
            }
            else check_all(vw, w, vx, x, n);
            if (n == 65 || n == THREE) { degenerate(n); refusals(vw, vx[0], n); }
            if (live() != before) die("the calls left vectors behind", n, live() - before);
        }
        rel(vw); for (V h : vx) rel(h);
    }
    if (sharded) return;
    // pending operands: the results against what the vectors hold once they exist
    const int64_t n = THREE;
    V stored = upload(data(n, 7, 0)), state = upload(data(n, 8, 1));
    V pending_w = 0, pending_x = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &pending_w));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, state, 1.0, &pending_x));
    V out = 0; double total = 0;
    OK(fmhip_resample(pending_w, FMHIP_RESAMPLE_SYSTEMATIC, n, 0.25, 0, &pending_x, 1, &out, nullptr, &total));
    {
        const F w = download(pending_w, n), x = download(pending_x, n), got = download(out, n);
        F want((size_t)n); const float* in[1] = { x.data() }; float* columns[1] = { want.data() }; double total_host = 0;
        OK(fmhip_resample_host(w.data(), n, FMHIP_RESAMPLE_SYSTEMATIC, n, 0.25, nullptr, in, 1, columns, nullptr, &total_host));
        if (std::memcmp(got.data(), want.data(), (size_t)n * 4) != 0 || total != total_host) die("a resample of pending vectors", n, 0);
    }
    rel(out); rel(stored); rel(state); rel(pending_w); rel(pending_x);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: a weighted call with one companion and the ancestors takes three pool allocations — two
// outputs and the temporary of P.  Without it this is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const F w = data(n, 5, 0), x = data(n, 6, 1);
    V vw = upload(w), vx = upload(x);
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out = 0, anc = 0; double total = -1.0;
        const int st = fmhip_resample(vw, FMHIP_RESAMPLE_SYSTEMATIC, n, 0.5, 0, &vx, 1, &out, &anc, &total);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) { rel(out); rel(anc); }
        else if (out != 0 || anc != 0 || total != -1.0) die("a failed call wrote its outputs", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a resample left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(vw); rel(vx);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: resample done\n", cycle);
        std::fflush(stdout);
    });
    if (plain) {                                                                // a device list of ONE shard is that shard's call
        const int device = 0;
        OK(fmhip_init_devices(&device, 1));
        scenario(false, false);
        OK(fmhip_shutdown());
        std::printf("a device list of one shard: checked\n");
    }
    return 0;
}
