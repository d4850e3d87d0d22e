// drive_prefix.cpp — drives fmhip_prefix_sums, fmhip_prefix_sums_at and fmhip_prefix_search through the C-ABI on the TEST-ONLY null device
// under the sanitizers.  The vectors hold real data and the stand-ins of null_prefix.cpp scan the chunks the plain way, so results are
// CHECKED against the definition (fmhip_prefix_sums_host): both modes of the output vector and the total, the prefixes at boundary
// positions (repeats, 4096 of them), the first crossings of thresholds at, below and above prefixes, relative ones, NaN — at n = 1, 65, one
// tile + 1, the smallest n with three workgroups and 300 007 (the scratch and the pinned stage grow between the calls), and 65 and 1 again
// behind the large one.  Pending operands, operands whose inputs another thread releases during the call, every argument error that is
// found on the host.  Twice, with a shutdown and a re-initialisation in between; then once more behind a device list of ONE shard.
// FMNULL_DEVICES=N: behind N shards every call is FMHIP_ERR_UNSUPPORTED and leaves nothing behind; FMNULL_THREAD_ENGINES=1: the calls come
// from a thread that does not own the vector.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_prefix_sums in which the allocation of the output fails.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"
#include "../../finmath-lib-cuda-extensions_amd/csrc/prefix_host.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(double a, double b) { return (a != a && b != b) || std::memcmp(&a, &b, 8) == 0; }
static bool same(float a, float b) { return (a != a && b != b) || std::memcmp(&a, &b, 4) == 0; }

// kind 0: weights over sixteen decades; kind 1: signed, with a NaN far behind
static F data(int64_t n, uint32_t seed, int kind) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (p % 5 == 2) x = 0.f;
        if (kind == 1) { if (s & 16u) x = -x; if (p == 250000) x = std::numeric_limits<float>::quiet_NaN(); }
        a[(size_t)p] = x;
    }
    if (kind == 0 && n > 3) a[0] = -0.f;
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static std::vector<double> definition(const F& a) { std::vector<double> p(a.size(), -1.0); OK(fmhip_prefix_sums_host(a.data(), (int64_t)a.size(), p.data())); return p; }
static int64_t live() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st.n_live_vectors; }

static void check_all(V v, const F& a) {
    const int64_t n = (int64_t)a.size();
    const std::vector<double> P = definition(a);
    for (int mode = 0; mode < 2; ++mode) {
        V out = 0; double total = -1.0;
        OK(fmhip_prefix_sums(v, mode, &out, mode ? nullptr : &total));
        const F got = download(out, n);
        for (int64_t r = 0; r < n; ++r) if (!same(got[(size_t)r], fm::prefix_out_host(P[(size_t)r], r, mode))) die("prefix sums", n, r);
        if (!mode && !same(total, P[(size_t)n - 1])) die("the total", n, 0);
        rel(out);
    }
    const int64_t tile = fm::FM_PREFIX_TILE, chunk = fm::prefix_chunk_elems(n);
    std::vector<int64_t> pos = { n - 1, 0, 0 };
    for (int64_t b : { (int64_t)7, (int64_t)8, (int64_t)63, (int64_t)64, (int64_t)511, (int64_t)512, tile - 1, tile, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk }) if (b < n) pos.push_back(b);
    for (int rounds = 0; rounds < 2; ++rounds) {
        std::vector<double> sums(pos.size(), -1.0);
        OK(fmhip_prefix_sums_at(v, pos.data(), (int)pos.size(), sums.data()));
        for (size_t j = 0; j < pos.size(); ++j) if (!same(sums[j], P[(size_t)pos[j]])) die("prefix sums at", n, (int64_t)j);
        pos.resize(fm::FM_PREFIX_MAX_QUERIES);                                   // 4096: the queries' table and the stage outgrow their first size
        for (size_t j = 0; j < pos.size(); ++j) pos[j] = (int64_t)((j * 7919u) % (uint64_t)n);
    }
    std::vector<double> ts = { -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), 0.0, P[0] };
    for (int64_t r : pos) { if (ts.size() > 600) break; const double x = P[(size_t)r]; ts.push_back(x); ts.push_back(std::nextafter(x, -1e300)); ts.push_back(std::nextafter(x, 1e300)); }
    for (int relative = 0; relative < 2; ++relative) {
        if (relative) ts = { 0.0, 0.5, 1.0, 0.25, 1.5, std::numeric_limits<double>::quiet_NaN(), -1.0 };
        std::vector<int64_t> where(ts.size(), -7); std::vector<double> sums(ts.size(), -1.0); double total = -1.0;
        OK(fmhip_prefix_search(v, ts.data(), (int)ts.size(), relative, where.data(), sums.data(), &total));
        if (!same(total, P[(size_t)n - 1])) die("the total of a search", n, relative);
        for (size_t j = 0; j < ts.size(); ++j) {
            const double t = relative ? ts[j] * P[(size_t)n - 1] : ts[j];
            const int64_t want = fm::prefix_search_host(P.data(), n, t);
            if (where[j] != want || !same(sums[j], want < n ? P[(size_t)want] : P[(size_t)n - 1])) die(relative ? "relative search" : "search", n, (int64_t)j);
        }
    }
    if (std::memcmp(download(v, n).data(), a.data(), (size_t)n * 4) != 0) die("the vector changed", n, 0);
}

static void refusals(V v, int64_t n, bool sharded) {
    const int64_t before = live();
    V out = 0; double sums[3], total = -1.0; int64_t where[3] = { -7, -7, -7 };
    const int64_t zero[1] = { 0 }; const double half[1] = { 0.5 };
    std::vector<int64_t> many((size_t)fm::FM_PREFIX_MAX_QUERIES + 1, 0); std::vector<double> many_t(many.size(), 0.0), many_s(many.size());
    EXPECT(fmhip_prefix_sums(v, 2, &out, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums(v, -1, &out, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums(v, 0, nullptr, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums(0, 0, &out, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums(v + 12345, 0, &out, &total), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_prefix_sums_at(v, zero, 0, sums), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums_at(v, many.data(), (int)many.size(), many_s.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums_at(v, nullptr, 1, sums), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums_at(v, zero, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums_at(0, zero, 1, sums), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_sums_at(v + 12345, zero, 1, sums), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_prefix_search(v, half, 0, 0, where, sums, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_search(v, many_t.data(), (int)many_t.size(), 0, many.data(), many_s.data(), &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_search(v, nullptr, 1, 0, where, sums, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_search(v, half, 1, 0, nullptr, sums, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_search(v, half, 1, 0, where, nullptr, &total), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_prefix_search(0, half, 1, 1, where, sums, &total), FMHIP_ERR_INVALID_ARGUMENT);
    // positions are looked at where the vector is: behind several shards the refusal of the list comes first
    const int64_t bad[4][3] = { { -1, 0, 0 }, { n, 0, 0 }, { 0, 5 % n, n }, { int64_t(1) << 40, 0, 0 } };
    for (const auto& b : bad) EXPECT(fmhip_prefix_sums_at(v, b, 3, sums), sharded ? FMHIP_ERR_UNSUPPORTED : FMHIP_ERR_INVALID_ARGUMENT);
    if (out != 0 || total != -1.0 || where[0] != -7 || live() != before) die("a refused call left something behind", n, live() - before);
}

static void unsupported(V v, int64_t n) {
    const int64_t before = live();
    V out = 0; double sums[2] = { -1.0, -1.0 }, total = -1.0; int64_t where[2] = { -7, -7 };
    const int64_t pos[2] = { 0, n - 1 }; const double ts[2] = { 0.5, 1.0 };
    EXPECT(fmhip_prefix_sums(v, 0, &out, &total), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_prefix_sums(v, 1, &out, nullptr), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_prefix_sums_at(v, pos, 2, sums), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_prefix_search(v, ts, 2, 1, where, sums, &total), FMHIP_ERR_UNSUPPORTED);
    if (out != 0 || total != -1.0 || sums[0] != -1.0 || where[0] != -7 || live() != before) die("a device list of several shards left something behind", n, live() - before);
}

static const int64_t THREE = [] { int64_t n = 2 * fm::prefix_chunk_elems(1) + 1; while (n % 64 == 0) ++n; return n; }();

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    if (fm::prefix_blocks(THREE) != 3 || fm::prefix_blocks(THREE - 1) != 2) die("the smallest n with three workgroups", THREE, 0);
    const int64_t sizes[7] = { 1, 65, fm::FM_PREFIX_TILE + 1, THREE, 300007, 65, 1 };
    for (int64_t n : sizes) {
        const F a = data(n, (uint32_t)n, 0), b = data(n, (uint32_t)n + 1, 1);
        V va = upload(a), vb = upload(b);
        if (sharded) { unsupported(va, n); if (n == 65) refusals(va, n, true); }
        else {
            const int64_t before = live();
            if (thread_engines) {
                std::thread asker([&] { check_all(va, a); check_all(vb, b); });      // a thread that owns neither
                asker.join();
                if (n < 300000) check_all(vb, b);                                   // and the owner
            }
            else { check_all(va, a); check_all(vb, b); }
            if (live() != before) die("the calls left vectors behind", n, live() - before);
            if (n == 65 || n == THREE) refusals(va, n, false);
        }
        rel(va); rel(vb);
    }
    if (sharded) return;
    // pending operands: statuses, and the results against what the vector holds once it exists
    const int64_t n = THREE;
    V stored = upload(data(n, 7, 0));
    V pending = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &pending));
    V out = 0; double total = 0;
    OK(fmhip_prefix_sums(pending, 0, &out, &total));
    {
        const std::vector<double> P = definition(download(pending, n));
        const F got = download(out, n);
        for (int64_t r = 0; r < n; ++r) if (!same(got[(size_t)r], (float)P[(size_t)r])) die("prefix sums of a pending vector", n, r);
        if (!same(total, P[(size_t)n - 1])) die("the total of a pending vector", n, 0);
    }
    rel(out);
    V again = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 3.0, &again));
    const int64_t pos[3] = { 0, n - 1, 0 }; double sums[3]; int64_t where[3]; const double ts[3] = { 0.0, 0.5, 1.0 };
    OK(fmhip_prefix_sums_at(again, pos, 3, sums));
    V third = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 4.0, &third));
    OK(fmhip_prefix_search(third, ts, 3, 1, where, sums, &total));
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handle keeps them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 8; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    OK(fmhip_prefix_sums(derived[0], 1, &out, nullptr));
    OK(fmhip_prefix_sums_at(derived[3], pos, 3, sums));
    OK(fmhip_prefix_search(derived[5], ts, 3, 1, where, sums, nullptr));
    releaser.join();
    rel(out);
    for (V d : derived) rel(d);
    rel(stored); rel(pending); rel(again); rel(third);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the output of one fmhip_prefix_sums is its one pool allocation.  Without it this is the
// counting run that says where it is.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5001;
    const F a = data(n, 5, 0);
    V v = upload(a);
    const std::vector<double> P = definition(a);
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out = 0; double total = -1.0;
        const int st = fmhip_prefix_sums(v, 0, &out, &total);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            const F got = download(out, n);
            for (int64_t r = 0; r < n; ++r) if (!same(got[(size_t)r], (float)P[(size_t)r])) die("prefix sums", n, r);
            rel(out);
        } else if (out != 0 || total != -1.0) die("a failed call wrote its outputs", n, 0);
        // the query calls take no buffer from the pool
        const int64_t pos[1] = { n - 1 }; double s = 0;
        OK(fmhip_prefix_sums_at(v, pos, 1, &s));
        if (!same(s, P[(size_t)n - 1])) die("prefix sums at", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a prefix_sums left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(v);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: prefix done\n", cycle);
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
