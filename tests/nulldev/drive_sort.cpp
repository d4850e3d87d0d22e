// drive_sort.cpp — drives fmhip_sort_by_key, fmhip_argsort, fmhip_rank_scores and fmhip_vec_read_elements through the C-ABI on the TEST-ONLY
// null device under the sanitizers.  The vectors hold real data (the read and write calls work on the null device) and the stand-ins of
// null_sort.cpp do the passes the plain way, so results are CHECKED: the permutation is fmhip_argsort_host's, every output of sort_by_key
// is a bit copy through it (0, 1 and 8 companions, the key among them, the same handle twice), the scores and the selected elements are
// right — at n = 1, 65, one tile + 1, the smallest n with three workgroups and 300 007 (the count table, the pinned stage and the scratch
// grow between the calls), and 65 and 1 again behind the large one.  Pending operands (the null device computes nothing element-wise:
// statuses, and the permutation against what the vector holds afterwards), operands whose inputs another thread releases during the call,
// every argument error that is found on the host.  Twice, with a shutdown and a re-initialisation in between; then once more behind a
// device list of ONE shard.  FMNULL_DEVICES=N: behind N shards every call is FMHIP_ERR_UNSUPPORTED and leaves nothing behind;
// FMNULL_THREAD_ENGINES=1: the calls come from a thread that owns none of the vectors, with owners mixed in one call.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one sort_by_key with 8 companions in which an allocation fails.
#include <cmath>
#include <string>
#include <thread>

#include "drive_common.hpp"
#include "../../finmath-lib-cuda-extensions_amd/csrc/sort_host.hpp"

typedef fmhip_vec V;
typedef std::vector<float> F;
static void rel(V h) { OK(fmhip_vec_release(h)); }
static void die(const char* what, int64_t n, int64_t at) { std::fprintf(stderr, "%s: n = %lld, at %lld\n", what, (long long)n, (long long)at); std::abort(); }

// ties, zeros of both signs, infinities, NaNs of several payloads; kind 1: every element its own bit pattern (a companion)
static F data(int64_t n, uint32_t seed, int kind) {
    F a((size_t)n);
    uint32_t s = seed * 2654435761u + 12345u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x;
        if (kind == 1) { const uint32_t u = (s & 0xFF800000u) | ((uint32_t)p & 0x007FFFFFu); std::memcpy(&x, &u, 4); }
        else {
            x = (float)(int32_t)(s >> 8) / 65536.0f - 128.0f;
            if (p % 3 == 1) x = std::floor(x / 16.0f);                       // ties
            if (p % 29 == 5) x = (s & 1u) ? -0.0f : 0.0f;
            if (p % 31 == 7) x = (s & 2u) ? INFINITY : -INFINITY;
            if (p % 37 == 11) { const uint32_t u = ((s & 4u) ? 0xFFC00000u : 0x7F800001u) + ((uint32_t)p & 0xFFFFu); std::memcpy(&x, &u, 4); }
        }
        a[(size_t)p] = x;
    }
    return a;
}
static V upload(const F& a) { V h = 0; OK(fmhip_vec_create_from_float(a.data(), (int64_t)a.size(), &h)); return h; }
static F download(V h, int64_t n) { F a((size_t)n); OK(fmhip_vec_read_float(h, a.data(), n)); return a; }
static std::vector<int64_t> definition(const F& a) { std::vector<int64_t> p(a.size(), -1); OK(fmhip_argsort_host(a.data(), (int64_t)a.size(), p.data())); return p; }
static int64_t live() { fmhip_pool_stats_t st; OK(fmhip_pool_stats(&st)); return st.n_live_vectors; }

static void same_bits(const F& got, const F& src, const std::vector<int64_t>& perm, const char* what) {
    for (size_t r = 0; r < perm.size(); ++r) if (std::memcmp(&got[r], &src[(size_t)perm[r]], 4) != 0) die(what, (int64_t)perm.size(), (int64_t)r);
}

// key, companions: handles and what they hold; every result against the definition
static void check_all(V key, const F& a, const std::vector<V>& vals, const std::vector<const F*>& held) {
    const int64_t n = (int64_t)a.size();
    const std::vector<int64_t> perm = definition(a);
    std::vector<int64_t> got((size_t)n, -1);
    OK(fmhip_argsort(key, got.data()));
    for (int64_t r = 0; r < n; ++r) if (got[(size_t)r] != perm[(size_t)r]) die("argsort", n, r);
    V sk = 0; std::vector<V> sv(vals.size() + 1, 0);
    OK(fmhip_sort_by_key(key, vals.empty() ? nullptr : vals.data(), (int)vals.size(), &sk, vals.empty() ? nullptr : sv.data()));
    same_bits(download(sk, n), a, perm, "sorted key");
    for (size_t i = 0; i < vals.size(); ++i) { same_bits(download(sv[i], n), *held[i], perm, "sorted companion"); rel(sv[i]); }
    rel(sk);
    if (!vals.empty()) {                                                       // without the key
        OK(fmhip_sort_by_key(key, vals.data(), (int)vals.size(), nullptr, sv.data()));
        for (size_t i = 0; i < vals.size(); ++i) { same_bits(download(sv[i], n), *held[i], perm, "sorted companion (no key)"); rel(sv[i]); }
    }
    V scores = 0;
    OK(fmhip_rank_scores(key, &scores));
    const F sc = download(scores, n);
    for (int64_t r = 0; r < n; ++r) { const float want = (float)(((double)r + 0.5) / (double)n); if (std::memcmp(&sc[(size_t)perm[(size_t)r]], &want, 4) != 0) die("rank scores", n, r); }
    rel(scores);
    const int count = n >= 300000 ? 70001 : 300;                                // 70 001: the positions' table and the stage outgrow their first size
    std::vector<int64_t> pos((size_t)count); std::vector<double> el((size_t)count, -1.0);
    for (int j = 0; j < count; ++j) pos[(size_t)j] = ((int64_t)j * 7919) % n;
    pos[0] = n - 1; pos[(size_t)count - 1] = 0; pos[(size_t)count / 2] = pos[1];
    OK(fmhip_vec_read_elements(key, pos.data(), count, el.data()));
    for (int j = 0; j < count; ++j) { const double want = (double)a[(size_t)pos[(size_t)j]]; if (!(el[(size_t)j] == want || (want != want && el[(size_t)j] != el[(size_t)j])) || std::signbit(el[(size_t)j]) != std::signbit(want)) die("read elements", n, j); }
    if (download(key, n) != a && std::memcmp(download(key, n).data(), a.data(), (size_t)n * 4) != 0) die("the key changed", n, 0);
}

static void refusals(V v, int64_t n, bool sharded) {
    V shorter = upload(data(n - 1, 3, 0));
    const int64_t before = live();
    V out_key = 0, out_vals[9] = { 0 };
    const V nine[9] = { v, v, v, v, v, v, v, v, v }, two[2] = { v, shorter }, none[1] = { 0 };
    EXPECT(fmhip_sort_by_key(v, nine, 9, &out_key, out_vals), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, nine, -1, &out_key, out_vals), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, nullptr, 0, nullptr, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, nullptr, 1, &out_key, out_vals), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, nine, 1, &out_key, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(0, nullptr, 0, &out_key, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, none, 1, &out_key, out_vals), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_sort_by_key(v, two, 2, &out_key, out_vals), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_sort_by_key(v + 12345, nullptr, 0, &out_key, nullptr), FMHIP_ERR_INVALID_HANDLE);
    EXPECT(fmhip_argsort(v, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_rank_scores(v, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    double out[3];
    const int64_t zero[1] = { 0 };
    EXPECT(fmhip_vec_read_elements(v, zero, 0, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_read_elements(v, nullptr, 1, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_vec_read_elements(v, zero, 1, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    // positions are looked at where the vector is: behind several shards the refusal of the list comes first
    const int64_t bad[4][3] = { { -1, 0, 0 }, { n, 0, 0 }, { 0, 5 % n, n }, { int64_t(1) << 40, 0, 0 } };
    for (const auto& b : bad) EXPECT(fmhip_vec_read_elements(v, b, 3, out), sharded ? FMHIP_ERR_UNSUPPORTED : FMHIP_ERR_INVALID_ARGUMENT);
    if (out_key != 0 || out_vals[0] != 0 || live() != before) die("a refused call left something behind", n, live() - before);
    rel(shorter);
}

static void unsupported(V key, V comp, int64_t n) {
    const int64_t before = live();
    std::vector<int64_t> perm((size_t)n, -1);
    V out = 0, outs[2] = { 0, 0 };
    const V both[2] = { comp, key };
    const int64_t pos[2] = { 0, n - 1 };
    double el[2];
    EXPECT(fmhip_argsort(key, perm.data()), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_sort_by_key(key, both, 2, &out, outs), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_sort_by_key(key, nullptr, 0, &out, nullptr), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_rank_scores(key, &out), FMHIP_ERR_UNSUPPORTED);
    EXPECT(fmhip_vec_read_elements(key, pos, 2, el), FMHIP_ERR_UNSUPPORTED);
    if (out != 0 || outs[0] != 0 || outs[1] != 0 || perm[0] != -1 || live() != before) die("a device list of several shards left something behind", n, live() - before);
}

static const int64_t THREE = [] { int64_t n = 2 * (int64_t)fm::sort_chunk_tiles(1) * fm::FM_SORT_TILE + 1; while (n % 64 == 0) ++n; return n; }();

static void scenario(bool thread_engines, bool sharded) {
    OK(fmhip_set_fusion(1, nullptr));
    if (fm::sort_blocks(THREE) != 3 || fm::sort_blocks(THREE - 1) != 2) die("the smallest n with three workgroups", THREE, 0);
    const int64_t sizes[7] = { 1, 65, fm::FM_SORT_TILE + 1, THREE, 300007, 65, 1 };
    for (int64_t n : sizes) {
        const F a = data(n, (uint32_t)n, 0);
        std::vector<F> c;
        for (int i = 0; i < 7; ++i) c.push_back(data(n, (uint32_t)(n + 1 + i), i & 1));
        V key = upload(a);
        std::vector<V> vals; std::vector<const F*> held;
        for (int i = 0; i < 7; ++i) { vals.push_back(i == 5 ? vals[2] : upload(c[(size_t)i])); held.push_back(i == 5 ? &c[2] : &c[(size_t)i]); }      // the same handle twice
        vals.push_back(key); held.push_back(&a);                                                                                                     // the key among them
        if (sharded) { unsupported(key, vals[0], n); if (n == 65) refusals(key, n, true); }
        else {
            const int64_t before = live();
            auto all = [&] {                                                   // (the large n: once, with everything)
                if (n < 300000) { check_all(key, a, {}, {}); check_all(key, a, { vals[1] }, { held[1] }); }
                check_all(key, a, vals, held);
            };
            if (thread_engines) {
                // a thread that owns none of them, and one call over vectors of two owners
                std::thread asker([&] {
                    all();
                    const F mine = data(n, 99, 1);
                    V m = upload(mine);
                    check_all(key, a, { vals[0], m, key }, { held[0], &mine, &a });
                    rel(m);
                });
                asker.join();
                if (n < 300000) check_all(key, a, { vals[1] }, { held[1] });      // and the owner, between the other thread's calls and the release
            }
            else all();
            if (live() != before) die("the calls left vectors behind", n, live() - before);
            if (n == 65 || n == THREE) refusals(key, n, false);
        }
        for (int i = 0; i < 7; ++i) if (i != 5) rel(vals[(size_t)i]);
        rel(key);
    }
    if (sharded) return;
    // pending operands: statuses, and the permutation against what the vector holds once it exists
    const int64_t n = THREE;
    V stored = upload(data(n, 7, 0));
    V pending = 0, pc = 0;
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0, &pc));
    std::vector<int64_t> got((size_t)n, -1);
    V sk = 0, sv[8] = { 0 };
    const V pcs[2] = { pc, stored };
    OK(fmhip_sort_by_key(pending, pcs, 2, &sk, sv));
    rel(sk); rel(sv[0]); rel(sv[1]);
    V again = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 3.0, &again));
    OK(fmhip_argsort(again, got.data()));
    const std::vector<int64_t> want = definition(download(again, n));
    for (int64_t r = 0; r < n; ++r) if (got[(size_t)r] != want[(size_t)r]) die("argsort of a pending vector", n, r);
    V third = 0, scores = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 4.0, &third));
    OK(fmhip_rank_scores(third, &scores)); rel(scores);
    V fourth = 0; OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 5.0, &fourth));
    const int64_t pos[3] = { 0, n - 1, 0 }; double el[3];
    OK(fmhip_vec_read_elements(fourth, pos, 3, el));
    // pending companions whose INPUTS another thread releases during the calls: only the call's own handles keep them computable
    std::vector<V> inputs, derived, garbage;
    for (int i = 0; i < 8; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    for (int i = 0; i < 64; ++i) { V g = 0; OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 100.0 + i, &g)); garbage.push_back(g); }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); for (V g : garbage) OK(fmhip_vec_release(g)); });
    OK(fmhip_sort_by_key(derived[0], derived.data(), 8, &sk, sv));
    OK(fmhip_argsort(derived[3], got.data()));
    releaser.join();
    rel(sk); for (V v : sv) rel(v);
    for (V d : derived) rel(d);
    rel(stored); rel(pending); rel(pc); rel(again); rel(third); rel(fourth);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the 4 ping-pong buffers and the 9 outputs of one sort_by_key are its 13 pool allocations.
// Without it this is the counting run that says where they are.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 3001;
    const F a = data(n, 5, 0);
    std::vector<F> c;
    for (int i = 0; i < 7; ++i) c.push_back(data(n, 50u + (uint32_t)i, 1));
    V key = upload(a);
    std::vector<V> vals;
    for (int i = 0; i < 7; ++i) vals.push_back(upload(c[(size_t)i]));
    vals.push_back(key);
    const std::vector<int64_t> perm = definition(a);
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V sk = 0, sv[8] = { 0 };
        const int st = fmhip_sort_by_key(key, vals.data(), 8, &sk, sv);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            same_bits(download(sk, n), a, perm, "sorted key");
            for (int i = 0; i < 8; ++i) { same_bits(download(sv[i], n), i == 7 ? a : c[(size_t)i], perm, "sorted companion"); rel(sv[i]); }
            rel(sk);
        } else if (sk != 0 || sv[0] != 0) die("a failed call wrote its outputs", n, 0);
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) die("a sort_by_key left something behind", after.n_live_vectors - before.n_live_vectors, after.bytes_in_use - before.bytes_in_use);
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    for (int i = 0; i < 7; ++i) rel(vals[(size_t)i]);
    rel(key);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    const bool plain = !std::getenv("FMNULL_DEVICES") && !std::getenv("FMNULL_THREAD_ENGINES");
    two_rounds([](int cycle, bool thread_engines, bool single_engine) {
        scenario(thread_engines, !thread_engines && !single_engine);
        std::printf("cycle %d: sort done\n", cycle);
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
