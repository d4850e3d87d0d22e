// producing_pass_host_time.cpp — what one call of each producing side pass costs the calling thread (profiles/producing_pass_frame.json):
// the ten calls at n = 4096 through the C-ABI on one engine, µs per call, median of `calls` calls after `warmup`, a host clock around the
// call alone.  The kernels are a few µs at this size, so the figure is the host's: checks, one flush, allocation, staging, launch, and —
// for the calls that wait — the wait.  Outputs are released and the stream is drained between calls, outside the clock.  The library is
// loaded from the path given, so that one binary measures two builds side by side:
//   g++ -O2 -std=c++17 -I include -o /tmp/ppht benchmarks/producing_pass_host_time.cpp -ldl
//   /tmp/ppht finmath-lib-cuda-extensions_amd/lib/libfmhip.so [calls=300] [warmup=30]      → one JSON line
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "fmhip.h"

static void* g_lib = nullptr;
template <class F> static F sym(const char* name) {
    void* p = dlsym(g_lib, name);
    if (!p) { std::fprintf(stderr, "%s: %s\n", name, dlerror()); std::exit(2); }
    return reinterpret_cast<F>(p);
}
#define FN(name) static const auto name##_ = sym<decltype(&name)>(#name)
#define OK(x) do { const int st_ = (x); if (st_ != FMHIP_OK) { std::fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #x, st_, fmhip_last_error_()); std::exit(1); } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s path/to/libfmhip.so [calls] [warmup]\n", argv[0]); return 2; }
    const int calls = argc > 2 ? std::atoi(argv[2]) : 300, warmup = argc > 3 ? std::atoi(argv[3]) : 30;
    g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) { std::fprintf(stderr, "%s\n", dlerror()); return 2; }
    FN(fmhip_last_error); FN(fmhip_init); FN(fmhip_shutdown); FN(fmhip_synchronize); FN(fmhip_vec_create_from_float); FN(fmhip_vec_release);
    FN(fmhip_polynomial_evaluate); FN(fmhip_binned_evaluate); FN(fmhip_sort_by_key); FN(fmhip_rank_scores); FN(fmhip_prefix_sums); FN(fmhip_table_build);
    FN(fmhip_table_apply); FN(fmhip_function_apply); FN(fmhip_option_formula); FN(fmhip_block_moments); FN(fmhip_vec_repeat);
    OK(fmhip_init_(-1));
    const int64_t n = 4096;
    uint64_t state = 88172645463325252ull;
    auto uniform = [&] { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (double)(state >> 11) / 9007199254740992.0; };
    auto column = [&](double lo, double hi) {
        std::vector<float> a((size_t)n);
        for (float& x : a) x = (float)(lo + (hi - lo) * uniform());
        fmhip_vec h = 0;
        OK(fmhip_vec_create_from_float_(a.data(), n, &h));
        return h;
    };
    const fmhip_vec key = column(-3.0, 3.0), x0 = column(-2.0, 2.0), x1 = column(-2.0, 2.0), u = column(0.01, 0.99), forward = column(0.5, 1.5), vol = column(0.1, 0.4);
    std::vector<fmhip_vec> made;                                                  // what the last call returned: released outside the clock
    const fmhip_vec states[2] = { x0, x1 }, extra[1] = { u }, bx[2] = { 0, x0 }, companions[2] = { x0, u }, two[2] = { x0, forward };
    const uint8_t exponents[6] = { 0, 0, 1, 2, 3, 0 };
    const double poly_c[4] = { 0.5, -1.25, 0.125, 2.0 }, bounds[3] = { -0.5, 0.0, 0.7 }, bin_c[8] = { 1.0, 2.0, -1.0, 0.5, 3.0, -2.0, 0.25, 1.0 };
    double knots[9], values[2][9], table_c[2 * 10 * 4];
    for (int k = 0; k < 9; ++k) { knots[k] = -2.0 + 0.5 * k; values[0][k] = std::sin(knots[k]); values[1][k] = knots[k] * knots[k]; }
    OK(fmhip_table_build_(knots, values[0], 9, FMHIP_TABLE_CUBIC_SPLINE, FMHIP_TABLE_LINEAR_EXTRAPOLATION, 0, table_c));
    OK(fmhip_table_build_(knots, values[1], 9, FMHIP_TABLE_LINEAR, FMHIP_TABLE_CONSTANT, 0, table_c + 40));
    const int kinds[3] = { FMHIP_FN_NORMAL_QUANTILE, FMHIP_FN_NORMAL_CDF, FMHIP_FN_NORMAL_DENSITY };
    struct Call { const char* name; std::function<int()> run; };
    const std::vector<Call> all = {
        { "polynomial_evaluate", [&] { made.assign(1, 0); return fmhip_polynomial_evaluate_(states, 2, exponents, 3, extra, 1, poly_c, made.data()); } },
        { "binned_evaluate", [&] { made.assign(1, 0); return fmhip_binned_evaluate_(key, bounds, 4, bx, 2, bin_c, made.data()); } },
        { "sort_by_key", [&] { made.assign(3, 0); return fmhip_sort_by_key_(key, companions, 2, made.data(), made.data() + 1); } },
        { "rank_scores", [&] { made.assign(1, 0); return fmhip_rank_scores_(x1, made.data()); } },
        { "prefix_sums", [&] { made.assign(1, 0); double total = 0; return fmhip_prefix_sums_(u, FMHIP_PREFIX_SUM, made.data(), &total); } },
        { "table_apply", [&] { made.assign(2, 0); return fmhip_table_apply_(x0, knots, 9, table_c, 2, made.data()); } },
        { "function_apply", [&] { made.assign(3, 0); return fmhip_function_apply_(u, kinds, 3, made.data()); } },
        { "option_formula", [&] { made.assign(3, 0); return fmhip_option_formula_(FMHIP_FORMULA_BLACK_SCHOLES, forward, 0.0, vol, 0.0, 0, 1.0, 2.0, 1.0, 7, made.data()); } },
        { "block_moments", [&] { made.assign(6, 0); return fmhip_block_moments_(two, 2, 64, 7u, made.data()); } },
        { "vec_repeat", [&] { made.assign(1, 0); return fmhip_vec_repeat_(x1, 2, 3, made.data()); } },
    };
    std::printf("{\"library\": \"%s\", \"n\": %lld, \"calls\": %d, \"median_us\": {", argv[1], (long long)n, calls);
    for (size_t c = 0; c < all.size(); ++c) {
        std::vector<double> us;
        for (int i = 0; i < warmup + calls; ++i) {
            const auto t0 = std::chrono::steady_clock::now();
            const int st = all[c].run();
            const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e6;
            OK(st);
            OK(fmhip_synchronize_());
            for (fmhip_vec h : made) OK(fmhip_vec_release_(h));
            if (i >= warmup) us.push_back(t);
        }
        std::sort(us.begin(), us.end());
        std::printf("%s\"%s\": %.2f", c ? ", " : "", all[c].name, 0.5 * (us[(us.size() - 1) / 2] + us[us.size() / 2]));
    }
    std::printf("}}\n");
    for (fmhip_vec h : { key, x0, x1, u, forward, vol }) OK(fmhip_vec_release_(h));
    OK(fmhip_shutdown_());
    return 0;
}
