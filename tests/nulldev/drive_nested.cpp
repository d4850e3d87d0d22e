// drive_nested.cpp — drives fmhip_block_moments and fmhip_vec_repeat through the C-ABI on the TEST-ONLY null device under the sanitizers.
// The vectors hold real data and the stand-ins of null_nested.cpp sum the blocks phase by phase, so results are CHECKED against the
// definition (fmhip_block_moments_host): every mask, one and four vectors per call, blocks of the three regimes and around their
// boundaries (1, 3, 64, 65, 2048, 2049, a block of several segments and a cut one; the scratch grows between the calls), a small shape
// again behind the large one; the repeat against the plain loop with NaN payloads and -0.0.  Pending operands, operands whose inputs
// another thread releases during the call, every argument error that is found on the host.  Twice, with a shutdown and a
// re-initialisation in between; then once more behind a device list of ONE shard.
// FMNULL_DEVICES=N: behind N shards every call is FMHIP_ERR_UNSUPPORTED and leaves nothing behind; FMNULL_THREAD_ENGINES=1: the calls come
// from a thread that does not own the vectors.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_block_moments in which the allocation of an output fails.
#include <cmath>
#include <limits>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// signed values over sixteen decades with zeros; special: a NaN with a payload, an infinity and a -0.0 in places of their own
static F data(int64_t n, uint32_t seed, bool special) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (p % 5 == 2) x = 0.f;
        if (s & 16u) x = -x;
        a[(size_t)p] = x;
    }
    if (special) {
        const uint32_t payload = 0x7fc12345u;
        std::memcpy(&a[0], &payload, 4);
        if (n > 2) a[(size_t)n / 2] = std::numeric_limits<float>::infinity();
        a[(size_t)n - 1] = -0.f;
    }
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static int64_t size_of(V h) { int64_t n = -1; OK(fmhip_vec_size(h, &n)); return n; }
static int64_t live() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st.n_live_vectors; }
static int bits(uint32_t mask) { return (int)((mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u)); }

static void check_moments(const std::vector<V>& vs, const std::vector<F>& as, int64_t block) {
    const int64_t n = (int64_t)as[0].size(), m = n / block;
    for (uint32_t mask = 1; mask <= 7; ++mask) {
        const int k = bits(mask);
        std::vector<V> outs(vs.size() * (size_t)k, 0);
        OK(fmhip_block_moments(vs.data(), (int)vs.size(), block, mask, outs.data()));
        for (size_t i = 0; i < vs.size(); ++i) {
            F want((size_t)(k * m), -1.f);
            OK(fmhip_block_moments_host(as[i].data(), n, block, mask, want.data()));
            for (int j = 0; j < k; ++j) {
                const V h = outs[i * (size_t)k + (size_t)j];
                if (size_of(h) != m) die("the size of an output", n, block);
                const F got = download(h, m);
                for (int64_t q = 0; q < m; ++q) if (!same(got[(size_t)q], want[(size_t)(j * m + q)])) die("block moments", block, q);
                rel(h);
            }
        }
    }
}

static void check_repeat(V v, const F& a, int64_t each, int64_t times) {
    const int64_t n = (int64_t)a.size(), total = n * each * times;
    V out = 0;
    OK(fmhip_vec_repeat(v, each, times, &out));
    if (size_of(out) != total) die("the size of a repeat", n, total);
    const F got = download(out, total);
    for (int64_t o = 0; o < total; ++o) if (!same(got[(size_t)o], a[(size_t)((o / each) % n)])) die("repeat", n, o);
    rel(out);
}

static void refusals(V v, V other_size, int64_t n) {
    const int64_t before = live();
    V outs[12] = { 0 }; V out = 0;
    const V two[2] = { v, v }, mixed[2] = { v, other_size }, with_zero[2] = { v, 0 }, five[5] = { v, v, v, v, v }, unknown[1] = { v + 12345 };
    EXPECT(fmhip_block_moments(two, 0, 1, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(five, 5, 1, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, 1, 0u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, 1, 8u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, 0, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, -3, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, n + 1, 7u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, n > 2 ? n - 1 : 2, 7u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(nullptr, 1, 1, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(two, 2, 1, 1u, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(with_zero, 2, 1, 1u, outs), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_block_moments(mixed, 2, 1, 1u, outs), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_block_moments(unknown, 1, 1, 1u, outs), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_vec_repeat(v, 0, 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, 1, 0, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, -1, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, (int64_t(1) << 31) / n + 1, 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, 1 << 16, (int64_t(1) << 15) / n + 1, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, int64_t(1) << 40, int64_t(1) << 40, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v, 2, 2, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(0, 2, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_repeat(v + 12345, 2, 2, &out), FMHIP_ERR_INVALID_HANDLE);
    if (outs[0] != 0 || out != 0 || live() != before) die("a refused call left something behind", n, live() - before);
}

static void unsupported(V v, int64_t n) {
    const int64_t before = live();
    V outs[12] = { 0 }; V out = 0;
    const V two[2] = { v, v };
    EXPECT(fmhip_block_moments(two, 2, 1, 7u, outs), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_block_moments(two, 1, n, 2u, outs), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_vec_repeat(v, 3, 2, &out), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_block_moments(two, 2, 1, 0u, outs), FMHIP_ERR_INVALID_ARGUMENT);      // what needs no look at a vector is still said first
    EXPECT(fmhip_vec_repeat(v, 0, 2, &out), FMHIP_ERR_INVALID_ARGUMENT);
    for (V h : outs) if (h != 0) die("a device list of several shards wrote an output", n, 0);
    if (out != 0 || live() != before) die("a device list of several shards left something behind", n, live() - before);
}

struct Shape { int64_t block, m; };

static void shapes_checked(bool four) {
    // small (1, 3, 64), medium (65, 2048), large (2049; 5 segments, the last one cut), then small again behind the grown scratch
    const Shape shapes[] = { { 1, 67 }, { 3, 23 }, { 64, 5 }, { 65, 3 }, { 2048, 2 }, { 2049, 3 }, { 4 * 2048 + 77, 2 }, { 7, 9 } };
    for (const Shape& sh : shapes) {
        const int64_t n = sh.block * sh.m;
        std::vector<F> as; std::vector<V> vs;
        for (int i = 0; i < (four ? 4 : 1); ++i) { as.push_back(data(n, (uint32_t)(n + i), i == 1)); vs.push_back(upload(as.back())); }
        const int64_t before = live();
        check_moments(vs, as, sh.block);
        if (live() != before) die("the calls left vectors behind", n, live() - before);
        for (V h : vs) rel(h);
    }
}

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 4097;
    const F a = data(n, 11, true), b = data(130, 12, false);
    V va = upload(a), vb = upload(b);
    if (sharded) { unsupported(va, n); unsupported(vb, 130); rel(va); rel(vb); return; }
    if (thread_engines) {
        std::thread asker([&] { shapes_checked(true); check_repeat(va, a, 3, 2); });      // a thread that owns none of va, vb
        asker.join();
        shapes_checked(false);
    } else { shapes_checked(true); shapes_checked(false); }
    const int64_t before = live();
    for (int64_t each : { 1, 2, 65 }) for (int64_t times : { 1, 3 }) { check_repeat(va, a, each, times); check_repeat(vb, b, each, times); }
    { const F one = data(1, 3, false); V v1 = upload(one); check_repeat(v1, one, 1000, 1); check_repeat(v1, one, 1, 1); rel(v1); }
    if (live() != before) die("the repeats left vectors behind", n, live() - before);
    refusals(va, vb, n);
    // pending operands: the results against what the vectors hold once they exist
    V p1 = 0, p2 = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, vb, 2.0, &p1));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 1.0, &p2));
    const V pend[2] = { p1, p2 }; V outs[4] = { 0 };
    OK(fmhip_block_moments(pend, 2, 13, 6u, outs));
    for (int i = 0; i < 2; ++i) {
        const F held = download(pend[i], 130); F want(20);
        OK(fmhip_block_moments_host(held.data(), 130, 13, 6u, want.data()));
        for (int j = 0; j < 2; ++j) { const F got = download(outs[i * 2 + j], 10); for (int q = 0; q < 10; ++q) if (!same(got[(size_t)q], want[(size_t)(j * 10 + q)])) die("block moments of a pending vector", 130, q); rel(outs[i * 2 + j]); }
    }
    V p3 = 0, rep = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, vb, 3.0, &p3));
    OK(fmhip_vec_repeat(p3, 4, 1, &rep));
    { const F held = download(p3, 130), got = download(rep, 520); for (int o = 0; o < 520; ++o) if (!same(got[(size_t)o], held[(size_t)(o / 4)])) die("repeat of a pending vector", 130, o); }
    rel(rep); rel(p1); rel(p2); rel(p3);
    // pending operands whose INPUTS another thread releases during the calls: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 6; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, vb, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    OK(fmhip_block_moments(derived.data(), 4, 10, 2u, outs));
    OK(fmhip_vec_repeat(derived[5], 2, 2, &rep));
    releaser.join();
    for (V h : outs) rel(h);
    rel(rep);
    for (V d : derived) rel(d);
    rel(va); rel(vb);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the outputs of one fmhip_block_moments are its pool allocations (six here).  Without it this
// is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 5000, block = 50, m = n / block;
    const F a = data(n, 5, false), b = data(n, 6, false);
    const V vs[2] = { upload(a), upload(b) };
    F want_a((size_t)(3 * m)), want_b((size_t)(3 * m));
    OK(fmhip_block_moments_host(a.data(), n, block, 7u, want_a.data()));
    OK(fmhip_block_moments_host(b.data(), n, block, 7u, want_b.data()));
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V outs[6] = { 0, 0, 0, 0, 0, 0 };
        const int st = fmhip_block_moments(vs, 2, block, 7u, outs);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            for (int k = 0; k < 6; ++k) {
                const F got = download(outs[k], m); const F& want = k < 3 ? want_a : want_b;
                for (int64_t q = 0; q < m; ++q) if (!same(got[(size_t)q], want[(size_t)((k % 3) * m + q)])) die("block moments", n, q);
                rel(outs[k]);
            }
        } else for (V h : outs) if (h != 0) die("a failed call wrote its outputs", n, 0);
        V rep = 0;
        const int rs = fmhip_vec_repeat(vs[0], 2, 1, &rep);
        if (rs == FMHIP_OK) rel(rep); else if (rep != 0) die("a failed repeat wrote its output", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a block_moments left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(vs[0]); rel(vs[1]);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: nested done\n", cycle);
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
