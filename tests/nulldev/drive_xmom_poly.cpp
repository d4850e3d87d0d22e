// drive_xmom_poly.cpp — drives fmhip_polynomial_cross_moments and fmhip_polynomial_evaluate through the C-ABI on the TEST-ONLY null device
// under the sanitizers, on vectors in every state a caller can hand over: stored, pending, rows that share storage, the constant 1 among the
// extra vectors and as the all-zero tuple, 1 … 8 states, 1 … 64 slots (one to four groups), with another thread releasing handles of PENDING
// operands' inputs while the call waits; then the errors that are found on the host.  Twice, with a shutdown and a re-initialisation in
// between.  FMNULL_DEVICES=N: behind a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread, the vectors asked
// about by a thread that does not own them.  The null device computes nothing element-wise, so a derived vector holds whatever its storage
// held; the two FILLED vectors have known values, and the stand-ins (null_xmom_poly.cpp) compute the definition where the engine expects
// it: every entry of S and T between regressors of known value is checked exactly — v_i·v_j·n with v a monomial of 1.5 and 0.5 —, which is
// a check of the slots the engine writes, of the layout it reads back and of the shard sums; the evaluation is read back and compared on
// every path; statuses are checked, the sanitizers do the rest.
// `failure` (with FMHIP_TEST_FAIL_ALLOC_AT set by the caller): one fmhip_polynomial_evaluate in which the allocation of the output fails.
#include <cmath>
#include <string>
#include <thread>

#include "drive_common.hpp"

typedef fmhip_vec V;
static V filled(int64_t n, double v) { V h = 0; OK(fmhip_vec_create_filled(n, v, &h)); return h; }
static void rel(V h) { OK(fmhip_vec_release(h)); }

// value[i]: what regressor / dependent i holds on every path, NaN where that is not known
static void ask(const std::vector<V>& states, const std::vector<uint8_t>& e, const std::vector<V>& extra, const std::vector<V>& y, const std::vector<double>& value, int64_t n) {
    const size_t nt = e.size() / states.size(), nx = nt + extra.size(), ny = y.size();
    std::vector<double> sums(nx * (nx + 1) / 2 + nx * ny, -1.0);
    OK(fmhip_polynomial_cross_moments(states.data(), (int)states.size(), e.data(), (int)nt, extra.empty() ? nullptr : extra.data(), (int)extra.size(), ny ? y.data() : nullptr, (int)ny, sums.data()));
    auto expect = [&](size_t a, size_t b, double got, const char* where) {
        if (std::isnan(value[a]) || std::isnan(value[b])) return;
        const double want = value[a] * value[b] * (double)n;               // multiples of 2^-12 below 2^53: exact in any order, over any shards
        if (got != want) { std::fprintf(stderr, "%s[%zu][%zu] = %g, expected %g\n", where, a, b, got, want); std::abort(); }
    };
    size_t at = 0;
    for (size_t i = 0; i < nx; ++i) for (size_t j = i; j < nx; ++j, ++at) expect(i, j, sums[at], "S");
    for (size_t i = 0; i < nx; ++i) for (size_t m = 0; m < ny; ++m, ++at) expect(i, nx + m, sums[at], "T");
}

static void scenario(bool thread_engines) {
    OK(fmhip_set_fusion(1, nullptr));
    const int64_t n = 2049;
    const double NaN = std::nan("");
    V stored = filled(n, 1.5), other = filled(n, 0.5);
    V pending = 0, twin = 0;
    OK(fmhip_call_v2s0(FMHIP_OP_ADD, stored, other, &pending));
    OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, stored, 2.0, &twin));
    std::vector<V> inputs, derived;
    for (int i = 0; i < 8; ++i) {
        V in = 0, d = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, stored, 1.0 + i, &in));
        OK(fmhip_call_v1s1(FMHIP_OP_MULT_S, in, 3.0, &d));
        inputs.push_back(in); derived.push_back(d);
    }
    std::thread releaser([&] { for (V g : inputs) OK(fmhip_vec_release(g)); });
    // three states (two known, one pending), every monomial of degree <= 3 in them: 20 terms; a term is known where the pending state has exponent 0
    const std::vector<V> three = { stored, other, pending };
    std::vector<uint8_t> e20; std::vector<double> v20;
    for (int a = 0; a <= 3; ++a) for (int b = 0; a + b <= 3; ++b) for (int c = 0; a + b + c <= 3; ++c) {
        e20.insert(e20.end(), { (uint8_t)a, (uint8_t)b, (uint8_t)c });
        v20.push_back(c ? NaN : std::pow(1.5, a) * std::pow(0.5, b));
    }
    auto with = [](std::vector<double> v, std::initializer_list<double> more) { v.insert(v.end(), more); return v; };
    const auto big = [&] {
        ask(three, e20, { 0, stored, derived[3] }, { other, pending, stored, twin }, with(v20, { 1.0, 1.5, NaN, 0.5, NaN, 1.5, NaN }), n);      // 27 slots: two groups
        std::vector<V> many_y(41, derived[1]); many_y.push_back(other);
        std::vector<double> v = with(v20, { 1.5, 1.0 }); v.insert(v.end(), 41, NaN); v.push_back(0.5);
        ask(three, e20, { stored, 0 }, many_y, v, n);                                                                                       // 64 slots: four groups
    };
    if (thread_engines) { std::thread asker(big); asker.join(); }          // vectors of another thread's engine
    big();
    ask({ stored }, { 1 }, {}, {}, { 1.5 }, n);
    ask({ stored }, { 0, 6, 1 }, {}, { other }, { 1.0, std::pow(1.5, 6), 1.5, 0.5 }, n);
    {   // eight states, the last with every exponent 0 … 6 in turn (max exponent per call varies)
        const std::vector<V> eight = { stored, other, stored, other, twin, derived[0], derived[5], other };
        std::vector<uint8_t> e; std::vector<double> v;
        for (int k = 0; k <= 6; ++k) { e.insert(e.end(), { 1, (uint8_t)(k & 1), 0, 0, 0, 0, 0, (uint8_t)k }); v.push_back(1.5 * std::pow(0.5, (k & 1) + k)); }
        e.insert(e.end(), { 0, 0, 0, 0, 1, 0, 2, 0 }); v.push_back(NaN);
        ask(eight, e, { other }, { stored }, with(v, { 0.5, 1.5 }), n);
    }
    releaser.join();
    {   // the fitted polynomial: 2 + 3·u·w² − u³ + 4·extra + 5 on known states, read back on every path
        const V states[2] = { stored, other }, extra[2] = { other, 0 };
        const uint8_t e[6] = { 0, 0, 1, 2, 3, 0 };
        const double c[5] = { 2.0, 3.0, -1.0, 4.0, 5.0 };
        V out = 0;
        OK(fmhip_polynomial_evaluate(states, 2, e, 3, extra, 2, c, &out));
        int64_t size = 0;
        OK(fmhip_vec_size(out, &size));
        std::vector<float> got((size_t)n);
        OK(fmhip_vec_read_float(out, got.data(), n));
        const float want = 2.0f + 3.0f * (1.5f * 0.25f) - 3.375f + 4.0f * 0.5f + 5.0f;
        for (int64_t p = 0; p < n; ++p) if (size != n || got[(size_t)p] != want) { std::fprintf(stderr, "evaluation: path %lld = %g, expected %g (size %lld)\n", (long long)p, got[(size_t)p], want, (long long)size); std::abort(); }
        V next = 0;
        OK(fmhip_call_v1s1(FMHIP_OP_ADD_S, out, 1.0, &next));                // the result is a vector like any other
        rel(next); rel(out);
    }
    // found on the host, before any launch
    std::vector<double> out(64 * 65 / 2 + 64 * 64);
    const std::vector<V> many(65, stored);
    const std::vector<uint8_t> ones(9 * 65, 1);
    const uint8_t seven[2] = { 7, 0 };
    const V zero[1] = { 0 }, with_zero[2] = { stored, 0 };
    V h = 0;
    const double c[64] = { 1.0 };
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, seven, 1, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 0, ones.data(), 1, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 9, ones.data(), 1, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 0, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 60, many.data(), 3, many.data(), 2, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, many.data(), -1, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(with_zero, 2, ones.data(), 3, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, nullptr, 0, zero, 1, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(nullptr, 2, ones.data(), 3, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, nullptr, 3, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, nullptr, 1, nullptr, 0, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, nullptr, 0, nullptr, 1, out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, nullptr, 0, nullptr, 0, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_evaluate(many.data(), 2, ones.data(), 58, many.data(), 3, c, &h), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_evaluate(many.data(), 2, ones.data(), 3, nullptr, 0, nullptr, &h), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_polynomial_evaluate(many.data(), 2, ones.data(), 3, nullptr, 0, c, nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    V shorter = filled(n - 1, 1.0);
    const V mixed[2] = { stored, shorter };
    EXPECT(fmhip_polynomial_cross_moments(mixed, 2, ones.data(), 3, nullptr, 0, nullptr, 0, out.data()), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, &shorter, 1, nullptr, 0, out.data()), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_polynomial_cross_moments(many.data(), 2, ones.data(), 3, nullptr, 0, &shorter, 1, out.data()), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_polynomial_evaluate(mixed, 2, ones.data(), 3, nullptr, 0, c, &h), FMHIP_ERR_SIZE_MISMATCH);
    EXPECT(fmhip_polynomial_cross_moments(&shorter, 1, ones.data(), 2, nullptr, 0, nullptr, 0, out.data()), FMHIP_OK);
    rel(shorter);
    for (V d : derived) rel(d);
    rel(stored); rel(other); rel(pending); rel(twin);
}

// FMHIP_TEST_FAIL_ALLOC_AT is set by the caller: the output of one fmhip_polynomial_evaluate is its one pool allocation.  Without it this
// is the counting run that says where it is.
static int failure() {
    OK(fmhip_init(0));
    const int64_t n = 2049;
    const V states[2] = { filled(n, 1.5), filled(n, 0.5) }, extra[2] = { states[1], 0 };
    const uint8_t e[6] = { 0, 0, 1, 2, 3, 0 };
    const double c[5] = { 2.0, 3.0, -1.0, 4.0, 5.0 };
    const float want = 2.0f + 3.0f * (1.5f * 0.25f) - 3.375f + 4.0f * 0.5f + 5.0f;
    std::vector<float> got((size_t)n);
    OK(fmhip_vec_read_float(states[0], got.data(), n));                      // (the filled vectors are stored before anything is counted)
    OK(fmhip_vec_read_float(states[1], got.data(), n));
    fmhip_pool_stats_t before, mid, after;
    OK(fmhip_pool_stats(&before));
    int first = -1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        V out = 0;
        const int st = fmhip_polynomial_evaluate(states, 2, e, 3, extra, 2, c, &out);
        if (attempt == 0) { first = st; OK(fmhip_pool_stats(&mid)); }
        if (st != FMHIP_OK && !(attempt == 0 && st == FMHIP_ERR_OUT_OF_MEMORY)) { std::fprintf(stderr, "attempt %d: status %d (%s)\n", attempt, st, fmhip_last_error()); std::abort(); }
        if (st == FMHIP_OK) {
            OK(fmhip_vec_read_float(out, got.data(), n));
            for (int64_t p = 0; p < n; ++p) if (got[(size_t)p] != want) { std::fprintf(stderr, "attempt %d: path %lld = %g, expected %g\n", attempt, (long long)p, got[(size_t)p], want); std::abort(); }
            rel(out);
        } else if (out != 0) { std::fprintf(stderr, "a failed call wrote its output\n"); std::abort(); }
        OK(fmhip_pool_stats(&after));
        if (after.n_live_vectors != before.n_live_vectors || after.bytes_in_use != before.bytes_in_use) {
            std::fprintf(stderr, "a polynomial_evaluate left %lld vectors and %lld bytes behind\n", (long long)(after.n_live_vectors - before.n_live_vectors), (long long)(after.bytes_in_use - before.bytes_in_use));
            std::abort();
        }
    }
    std::printf("failure: %lld allocations before the call, %lld in it, status %d\n", (long long)(before.n_alloc_hits + before.n_alloc_misses),
                (long long)(mid.n_alloc_hits + mid.n_alloc_misses - before.n_alloc_hits - before.n_alloc_misses), first);
    rel(states[0]); rel(states[1]);
    OK(fmhip_shutdown());
    std::printf("failure done\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "failure") return failure();
    return two_rounds([](int cycle, bool thread_engines, bool) {
        scenario(thread_engines);
        std::printf("cycle %d: xmom poly done\n", cycle);
        std::fflush(stdout);
    });
}
