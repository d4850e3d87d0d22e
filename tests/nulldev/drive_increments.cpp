// drive_increments.cpp — drives fmhip_increments_generate_device through the C-ABI on the TEST-ONLY null device under the sanitizers: whole
// processes and blocks behind a path offset (one engine; FMNULL_DEVICES=N: behind a device list of N shards, every shard its own block;
// FMNULL_THREAD_ENGINES=1: an engine per caller thread), downloaded and compared with fmhip_increments_host narrowed to fp32 — the stand-in
// launcher (null_mt.cpp) generates with the host code from the state, the descriptors and the tables the engine hands it, so what is
// checked is the engine: seeding, jump distances, tables shared between equal means, the layout of descriptors, tables and slab, the
// handles; then the errors that are found on the host, with another thread creating and releasing vectors meanwhile.  Twice, with a
// shutdown and a re-initialisation in between.
#include <atomic>
#include <cmath>
#include <thread>

#include "drive_common.hpp"

namespace fm { extern std::atomic<int> g_null_icdf_tables, g_null_icdf_table_doubles; }

struct Laws {
    int steps, factors;
    std::vector<int32_t> kind; std::vector<double> a, b;
    Laws(int steps_, int factors_) : steps(steps_), factors(factors_), kind((size_t)steps_ * factors_), a(kind.size()), b(kind.size()) {}
    void set(int step, int factor, int32_t k, double a_, double b_ = 0.0) { const size_t i = (size_t)step * factors + factor; kind[i] = k; a[i] = a_; b[i] = b_; }
};

// the three factors of a Merton model over the given time steps
static Laws merton(const std::vector<double>& dt, double intensity) {
    Laws L((int)dt.size(), 3);
    for (int i = 0; i < L.steps; ++i) { L.set(i, 0, FMHIP_LAW_NORMAL, std::sqrt(dt[(size_t)i])); L.set(i, 1, FMHIP_LAW_NORMAL, 1.0); L.set(i, 2, FMHIP_LAW_POISSON, intensity * dt[(size_t)i]); }
    return L;
}

static void block(int32_t seed, const Laws& L, int64_t n, int64_t offset) {
    compare_block(seed, L.kind.size(), n, offset,
                  [&](fmhip_vec* h) { return fmhip_increments_generate_device(seed, L.steps, L.factors, n, offset, L.kind.data(), L.a.data(), L.b.data(), h); },
                  [&](double* host) { return fmhip_increments_host(seed, L.steps, L.factors, offset + n, L.kind.data(), L.a.data(), L.b.data(), host); });
}

static void scenario(bool thread_engines, bool single_engine) {
    const std::vector<double> dt = { 0.25, 0.0, 1.5, 0.25 };
    std::thread churn([] {                                  // another caller of the same process meanwhile
        for (int i = 0; i < 200; ++i) { fmhip_vec v = 0; OK(fmhip_vec_create_filled(100 + i, 1.0, &v)); OK(fmhip_vec_release(v)); }
    });
    const Laws m = merton(dt, 2.0);
    block(31415, m, 1000, 0);
    if (single_engine && (fm::g_null_icdf_tables != 3 || fm::g_null_icdf_table_doubles < 3)) {      // means 0.5 (twice), 0 and 3: three tables for four Poisson laws
        std::fprintf(stderr, "%d tables of %d doubles were uploaded, expected 3\n", fm::g_null_icdf_tables.load(), fm::g_null_icdf_table_doubles.load()); std::abort();
    }
    block(-7, m, 1, 0);
    block(31415, m, 0, 12);
    block(31415, m, 333, 1);                                // an odd offset
    block(31415, m, 5, 20001);                              // 480 024 words in front: several table rows
    Laws mixed(2, 2);
    mixed.set(0, 0, FMHIP_LAW_UNIFORM, -1.0, 3.0); mixed.set(0, 1, FMHIP_LAW_POISSON, 128.0);
    mixed.set(1, 0, FMHIP_LAW_POISSON, 0.02); mixed.set(1, 1, FMHIP_LAW_UNIFORM, 2.0, 2.0);
    block(1, mixed, 4097, 3);
    Laws normal(1, 1); normal.set(0, 0, FMHIP_LAW_NORMAL, 1.0);
    block(1, normal, 100, 0);                               // no Poisson law: an empty table block
    Laws many(50, 1);                                       // a mean per step
    for (int i = 0; i < 50; ++i) many.set(i, 0, FMHIP_LAW_POISSON, 0.1 * i);
    block(5, many, 200, 7);
    if (thread_engines) { std::thread other([&] { block(99, m, 777, 5); }); other.join(); }
    churn.join();

    fmhip_vec out[12];
    const Laws ok = merton(dt, 2.0);
    auto with = [&](int i, int32_t k, double a, double b) { Laws L = ok; L.kind[(size_t)i] = k; L.a[(size_t)i] = a; L.b[(size_t)i] = b; return L; };
    const double nan = std::nan(""), inf = HUGE_VAL;
    const Laws bad[] = { with(4, 3, 1.0, 0.0), with(4, -1, 1.0, 0.0), with(0, FMHIP_LAW_NORMAL, -1.0, 0.0), with(0, FMHIP_LAW_NORMAL, nan, 0.0),
                         with(5, FMHIP_LAW_POISSON, -0.5, 0.0), with(5, FMHIP_LAW_POISSON, nan, 0.0), with(5, FMHIP_LAW_POISSON, 128.5, 0.0),
                         with(7, FMHIP_LAW_UNIFORM, 2.0, 1.0), with(7, FMHIP_LAW_UNIFORM, 0.0, inf), with(7, FMHIP_LAW_UNIFORM, nan, 1.0) };
    std::vector<double> host(12 * 10);
    for (const Laws& L : bad) {
        EXPECT(fmhip_increments_generate_device(1, L.steps, L.factors, 10, 0, L.kind.data(), L.a.data(), L.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
        EXPECT(fmhip_increments_host(1, L.steps, L.factors, 10, L.kind.data(), L.a.data(), L.b.data(), host.data()), FMHIP_ERR_INVALID_ARGUMENT);
    }
    EXPECT(fmhip_increments_generate_device(1, 0, 3, 10, 0, ok.kind.data(), ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 0, 10, 0, ok.kind.data(), ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, -1, 0, ok.kind.data(), ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, -1, ok.kind.data(), ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, 0, nullptr, ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, 0, ok.kind.data(), nullptr, ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, 0, ok.kind.data(), ok.a.data(), nullptr, out), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, 0, ok.kind.data(), ok.a.data(), ok.b.data(), nullptr), FMHIP_ERR_INVALID_ARGUMENT);
    EXPECT(fmhip_increments_generate_device(1, 4, 3, 10, (int64_t(1) << 44) / 24, ok.kind.data(), ok.a.data(), ok.b.data(), out), FMHIP_ERR_INVALID_ARGUMENT);
    Laws tables(400, 1);                                    // 400 distinct means near 100: more than 2^16 table doubles
    for (int i = 0; i < 400; ++i) tables.set(i, 0, FMHIP_LAW_POISSON, 100.0 + 1e-3 * i);
    std::vector<fmhip_vec> many_out(400);
    EXPECT(fmhip_increments_generate_device(1, 400, 1, 10, 0, tables.kind.data(), tables.a.data(), tables.b.data(), many_out.data()), FMHIP_ERR_INVALID_ARGUMENT);
    std::printf("increments done\n");
}

int main() { return two_rounds([](int, bool thread_engines, bool single_engine) { scenario(thread_engines, single_engine); }); }
