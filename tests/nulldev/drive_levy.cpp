// drive_levy.cpp — drives fmhip_increments_generate_device with gamma and exponential laws through the C-ABI on the TEST-ONLY null device
// under the sanitizers, as drive_increments.cpp does for the three older laws: whole processes and blocks behind a path offset (one engine;
// FMNULL_DEVICES=N: a device list of N shards; FMNULL_THREAD_ENGINES=1: an engine per caller thread), downloaded and compared with
// fmhip_increments_host narrowed to fp32.  The stand-in (null_mt_levy.cpp) generates from the state, the descriptors and the constants the
// engine hands it, so what is checked is the engine: which launcher it picks, seeding, jump distances, one entry of constants per distinct
// shape beside the Poisson tables, the layout; then the new argument errors.  Twice, with a shutdown and a re-initialisation in between.
#include <atomic>
#include <cmath>
#include <thread>

#include "drive_common.hpp"

namespace fm { extern std::atomic<int> g_null_levy_launches, g_null_levy_entries, g_null_levy_doubles, g_null_icdf_tables; }

struct Laws {
    int steps, factors;
    std::vector<int32_t> kind; std::vector<double> a, b;
    Laws(int steps_, int factors_) : steps(steps_), factors(factors_), kind((size_t)steps_ * factors_), a(kind.size()), b(kind.size()) {}
    void set(int step, int factor, int32_t k, double a_, double b_ = 0.0) { const size_t i = (size_t)step * factors + factor; kind[i] = k; a[i] = a_; b[i] = b_; }
};

static Laws variance_gamma(const std::vector<double>& dt, double nu) {
    Laws L((int)dt.size(), 2);
    for (int i = 0; i < L.steps; ++i) { L.set(i, 0, FMHIP_LAW_GAMMA, dt[(size_t)i] / nu, nu); L.set(i, 1, FMHIP_LAW_NORMAL, 1.0); }
    return L;
}

static void block(int32_t seed, const Laws& L, int64_t n, int64_t offset) {
    compare_block(seed, L.kind.size(), n, offset,
                  [&](fmhip_vec* h) { return fmhip_increments_generate_device(seed, L.steps, L.factors, n, offset, L.kind.data(), L.a.data(), L.b.data(), h); },
                  [&](double* host) { return fmhip_increments_host(seed, L.steps, L.factors, offset + n, L.kind.data(), L.a.data(), L.b.data(), host); });
}

static void scenario(bool thread_engines, bool single_engine) {
    const std::vector<double> dt = { 0.25, 0.0125, 1.5, 0.25 };
    std::thread churn([] {
        for (int i = 0; i < 200; ++i) { fmhip_vec v = 0; OK(fmhip_vec_create_filled(100 + i, 1.0, &v)); OK(fmhip_vec_release(v)); }
    });
    const Laws vg = variance_gamma(dt, 0.2);
    const int before = fm::g_null_levy_launches;
    block(31415, vg, 1000, 0);
    if (single_engine && (fm::g_null_levy_launches != before + 1 || fm::g_null_levy_entries != 3 || fm::g_null_levy_doubles != 18)) {   // shapes 1.25 (twice), 0.0625 and 7.5
        std::fprintf(stderr, "%d launches, %d entries of %d doubles, expected 1, 3, 18\n", fm::g_null_levy_launches - before, fm::g_null_levy_entries.load(), fm::g_null_levy_doubles.load()); std::abort();
    }
    block(-7, vg, 1, 0);
    block(31415, vg, 0, 12);
    block(31415, vg, 333, 1);
    block(31415, vg, 5, 20001);
    Laws mixed(2, 3);                                      // all five laws; a Poisson table between two entries of constants
    mixed.set(0, 0, FMHIP_LAW_GAMMA, 0.01, 3.0); mixed.set(0, 1, FMHIP_LAW_POISSON, 2.0); mixed.set(0, 2, FMHIP_LAW_EXPONENTIAL, 4.0);
    mixed.set(1, 0, FMHIP_LAW_UNIFORM, -1.0, 3.0); mixed.set(1, 1, FMHIP_LAW_GAMMA, 1000.0, 1e-3); mixed.set(1, 2, FMHIP_LAW_NORMAL, 0.5);
    block(1, mixed, 4097, 3);
    Laws exponential(1, 1); exponential.set(0, 0, FMHIP_LAW_EXPONENTIAL, 0.5);
    block(1, exponential, 100, 0);                         // no table entry at all
    Laws many(50, 1);                                      // a shape per step
    for (int i = 0; i < 50; ++i) many.set(i, 0, FMHIP_LAW_GAMMA, 0.05 + 0.7 * i, 1.0 + i);
    block(5, many, 200, 7);
    if (single_engine) {                                    // the old laws alone do not come here
        const int launches = fm::g_null_levy_launches;
        Laws old(1, 2); old.set(0, 0, FMHIP_LAW_NORMAL, 1.0); old.set(0, 1, FMHIP_LAW_POISSON, 1.0);
        block(3, old, 50, 0);
        if (fm::g_null_levy_launches != launches) { std::fprintf(stderr, "a call with the old laws only ran the new kernel\n"); std::abort(); }
    }
    if (thread_engines) { std::thread other([&] { block(99, vg, 777, 5); }); other.join(); }
    churn.join();

    fmhip_vec out[8];
    auto with = [&](int i, int32_t k, double a, double b) { Laws L = vg; L.kind[(size_t)i] = k; L.a[(size_t)i] = a; L.b[(size_t)i] = b; return L; };
    const double nan = std::nan(""), inf = HUGE_VAL;
    const Laws bad[] = { with(4, 3, 1.0, 0.0), with(4, 6, 1.0, 1.0),
                         with(0, FMHIP_LAW_GAMMA, 0.0, 1.0), with(0, FMHIP_LAW_GAMMA, -1.0, 1.0), with(0, FMHIP_LAW_GAMMA, nan, 1.0), with(0, FMHIP_LAW_GAMMA, inf, 1.0),
                         with(2, FMHIP_LAW_GAMMA, 0.009, 1.0), with(2, FMHIP_LAW_GAMMA, 1000.5, 1.0),
                         with(6, FMHIP_LAW_GAMMA, 1.0, 0.0), with(6, FMHIP_LAW_GAMMA, 1.0, -1.0), with(6, FMHIP_LAW_GAMMA, 1.0, nan), with(6, FMHIP_LAW_GAMMA, 1.0, inf),
                         with(5, FMHIP_LAW_EXPONENTIAL, 0.0, 0.0), with(5, FMHIP_LAW_EXPONENTIAL, -2.0, 0.0), with(5, FMHIP_LAW_EXPONENTIAL, nan, 0.0), with(5, FMHIP_LAW_EXPONENTIAL, inf, 0.0) };
    std::vector<double> host(8 * 10);
    for (const Laws& L : bad) {
        EXPECT(fmhip_increments_generate_device(1, L.steps, L.factors, 10, 0, L.kind.data(), L.a.data(), L.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_increments_host(1, L.steps, L.factors, 10, L.kind.data(), L.a.data(), L.b.data(), host.data()), FMHIP_ERR_INVALID_ARGUMENT);
    }
    Laws shapes(10923, 1);                                  // 10 923 distinct shapes of 6 constants: more than 2^16 table doubles
    for (int i = 0; i < 10923; ++i) shapes.set(i, 0, FMHIP_LAW_GAMMA, 1.0 + 1e-4 * i, 1.0);
    std::vector<fmhip_vec> many_out(10923);
    EXPECT(fmhip_increments_generate_device(1, 10923, 1, 10, 0, shapes.kind.data(), shapes.a.data(), shapes.b.data(), many_out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    std::printf("levy done\n");
}

int main() { return two_rounds([](int, bool thread_engines, bool single_engine) { scenario(thread_engines, single_engine); }); }
