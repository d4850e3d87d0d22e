// test_group_host.cpp — the definition of the device reduce-by-key (csrc/group_host.hpp) on the CPU, stand-alone, built with
// -fsanitize=address,undefined by tests/test_group_cpu.py.  Every consequence the header states is an equality or a bound here:
//   one group is the prefix total of prefix_sums_host bit for bit; a group of one member is that member (a lone -0.0 stays -0.0); the bits of
//   a group do not depend on the values of other groups, on n_values, a vector's slot or the mask; the fp64 bound against an exact (long
//   double) sum of the group's own terms; a NaN or ±inf stays inside its group; membership, counts and `ungrouped` for hostile indices; the
//   empty group; the argument complaints.
#include "../../finmath-lib-cuda-extensions_amd/csrc/group_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <random>

using namespace fm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); if (++failures > 20) std::exit(1); } } while (0)

static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
static void refused(const std::function<void()>& f, const char* what) {
    try { f(); } catch (const std::invalid_argument&) { return; }
    std::printf("FAILED: not refused: %s\n", what); ++failures;
}

struct Doubles { std::vector<int64_t> counts; std::vector<double> s1, s2; int64_t ungrouped = -1; };
static Doubles sums(const std::vector<float>& index, int64_t m, const std::vector<float>& v) {
    Doubles d; d.counts.resize((size_t)m); d.s1.resize((size_t)m); d.s2.resize((size_t)m);
    const float* in = v.data(); double* a = d.s1.data(); double* b = d.s2.data();
    group_sums_double_host(index.data(), (int64_t)index.size(), m, &in, 1, d.counts.data(), &a, &b, &d.ungrouped);
    return d;
}

static void one_group_is_the_prefix_total(std::mt19937& rng) {
    std::normal_distribution<float> normal(0.5f, 3.0f);
    for (int64_t n : { 1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 12289, 100003, 4194305 }) {
        std::vector<float> v((size_t)n), index((size_t)n, 0.0f);
        for (float& x : v) x = normal(rng);
        std::vector<double> p((size_t)n);
        prefix_sums_host(v.data(), n, p.data());
        const Doubles d = sums(index, 1, v);
        CHECK(bits(d.s1[0]) == bits(p[(size_t)n - 1]) && d.counts[0] == n && d.ungrouped == 0);
        // … and the run-prefixes are P at every position: the heads of one run add nothing to the rule
        std::vector<double> q((size_t)n);
        std::vector<unsigned char> head((size_t)n, 0); head[0] = 1;
        for (int64_t r = 0; r < n; ++r) q[(size_t)r] = (double)v[(size_t)r];
        group_unit_host(q.data(), head.data(), n, 6, prefix_chunk_elems(n));
        bool same = true;
        for (int64_t r = 0; r < n; ++r) same = same && bits(q[(size_t)r]) == bits(p[(size_t)r]);
        CHECK(same);
    }
}

static void single_members_and_minus_zero() {
    const int64_t n = 5000;
    std::vector<float> index((size_t)n), v((size_t)n);
    for (int64_t j = 0; j < n; ++j) { index[(size_t)j] = (float)(n - 1 - j); v[(size_t)j] = j % 3 == 0 ? -0.0f : (float)j * 0.37f - 11.0f; }      // a permutation
    const Doubles d = sums(index, n, v);
    for (int64_t j = 0; j < n; ++j) {
        const double x = (double)v[(size_t)j];
        CHECK(d.counts[(size_t)(n - 1 - j)] == 1 && bits(d.s1[(size_t)(n - 1 - j)]) == bits(x) && bits(d.s2[(size_t)(n - 1 - j)]) == bits(x * x));
    }
    std::vector<float> counts((size_t)n), out((size_t)n);
    const float* in = v.data(); float* o = out.data();
    group_sums_host(index.data(), n, n, &in, 1, fmhost::FM_BLOCK_SUM, counts.data(), &o, nullptr);
    for (int64_t j = 0; j < n; ++j) CHECK(bits(out[(size_t)(n - 1 - j)]) == bits(v[(size_t)j]) && counts[(size_t)j] == 1.0f);
}

// heads on and one either side of the lane, group, wave, tile and chunk boundaries: sorted runs
static std::vector<float> runs_index(int64_t n, const std::vector<int64_t>& heads) {
    std::vector<float> index((size_t)n);
    size_t h = 0; int64_t k = 0;
    for (int64_t r = 0; r < n; ++r) { if (h < heads.size() && heads[h] == r) { if (r > 0) ++k; ++h; } index[(size_t)r] = (float)k; }
    return index;
}

static void the_bound_and_independence(std::mt19937& rng) {
    std::normal_distribution<float> normal(0.0f, 100.0f);
    std::vector<int64_t> heads{ 0 };
    for (int64_t b : { 8, 64, 512, 2048, 4096, 8192 }) for (int64_t d : { -1, 0, 1 }) heads.push_back(b + d);
    std::sort(heads.begin(), heads.end());
    for (int64_t n : { 9000, 12289, 100003 }) {
        for (int family = 0; family < 2; ++family) {
            std::vector<float> index = runs_index(n, heads);
            int64_t m = (int64_t)index.back() + 1;
            if (family == 1) { m = 37; std::uniform_int_distribution<int> u(0, 36); for (float& x : index) x = (float)u(rng); }
            std::vector<float> v((size_t)n);
            for (float& x : v) x = normal(rng);
            const Doubles d = sums(index, m, v);
            // the bound, relative to the group's own terms
            std::vector<long double> exact1((size_t)m, 0.0L), exact2((size_t)m, 0.0L), abs1((size_t)m, 0.0L);
            std::vector<int64_t> counts((size_t)m, 0);
            for (int64_t j = 0; j < n; ++j) {
                const size_t k = (size_t)index[(size_t)j]; const long double x = (long double)v[(size_t)j];
                exact1[k] += x; exact2[k] += x * x; abs1[k] += std::fabs(x); counts[k]++;
            }
            const long double eps = (long double)(prefix_chain(n) + 1) * std::ldexp(1.0L, -53);
            for (int64_t k = 0; k < m; ++k) {
                CHECK(d.counts[(size_t)k] == counts[(size_t)k]);
                // (the long double sums carry an error of their own: 2^-64 per addition, far below the bound)
                CHECK(std::fabs((long double)d.s1[(size_t)k] - exact1[(size_t)k]) <= eps * abs1[(size_t)k] * 1.001L);
                CHECK(std::fabs((long double)d.s2[(size_t)k] - exact2[(size_t)k]) <= eps * exact2[(size_t)k] * 1.001L);
            }
            // other groups' values — NaN and ±inf among them — leave a group's bits alone
            std::vector<float> w = v;
            const float odd[4] = { std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 1e30f };
            for (int64_t j = 0; j < n; ++j) if ((int64_t)index[(size_t)j] % 2 == 1) w[(size_t)j] = odd[j % 4];
            const Doubles e = sums(index, m, w);
            for (int64_t k = 0; k < m; k += 2) CHECK(bits(e.s1[(size_t)k]) == bits(d.s1[(size_t)k]) && bits(e.s2[(size_t)k]) == bits(d.s2[(size_t)k]));
            // one NaN inside a group is that group's alone
            std::vector<float> z = v; z[(size_t)(n / 2)] = odd[0];
            const Doubles f = sums(index, m, z);
            for (int64_t k = 0; k < m; ++k) {
                if (k == (int64_t)index[(size_t)(n / 2)]) CHECK(f.s1[(size_t)k] != f.s1[(size_t)k]);
                else CHECK(bits(f.s1[(size_t)k]) == bits(d.s1[(size_t)k]));
            }
            // n_values, the slot and the mask: the float outputs of four vectors under every mask are those of each vector alone
            std::vector<float> x3((size_t)n); for (float& x : x3) x = normal(rng);
            const float* four[4] = { w.data(), v.data(), x3.data(), v.data() };
            for (uint32_t mask = 1; mask <= 7; ++mask) {
                const int per = fmhost::fm_block_outputs(mask);
                std::vector<std::vector<float>> outs((size_t)(4 * per), std::vector<float>((size_t)m)), alone((size_t)per, std::vector<float>((size_t)m));
                std::vector<float*> po, pa;
                for (auto& o : outs) po.push_back(o.data());
                for (auto& o : alone) pa.push_back(o.data());
                group_sums_host(index.data(), n, m, four, 4, mask, nullptr, po.data(), nullptr);
                const float* in = v.data();
                group_sums_host(index.data(), n, m, &in, 1, mask, nullptr, pa.data(), nullptr);
                int j = 0;
                for (int bit = 1; bit <= 4; bit <<= 1) {
                    if (!(mask & (uint32_t)bit)) continue;
                    bool same = true;
                    for (int64_t k = 0; k < m; ++k) {
                        same = same && bits(outs[(size_t)(per + j)][(size_t)k]) == bits(alone[(size_t)j][(size_t)k]) && bits(outs[(size_t)(3 * per + j)][(size_t)k]) == bits(alone[(size_t)j][(size_t)k]);
                        same = same && bits(alone[(size_t)j][(size_t)k]) == bits(group_output(bit, d.s1[(size_t)k], d.s2[(size_t)k], d.counts[(size_t)k]));
                    }
                    CHECK(same);
                    ++j;
                }
            }
        }
    }
}

static void membership_and_the_empty_group() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int64_t m = 4;
    const std::vector<float> index{ nan, inf, -inf, -1.0f, 0.5f, (float)m, 1073741824.0f, -0.0f, 0.0f, 3.0f, 2.9999998f, 3.0f };
    const std::vector<float> v{ 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12 };
    const Doubles d = sums(index, m, v);
    CHECK(d.ungrouped == 8 && d.counts[0] == 2 && d.counts[1] == 0 && d.counts[2] == 0 && d.counts[3] == 2);
    CHECK(d.s1[0] == 17.0 && d.s1[3] == 22.0 && d.s2[3] == 244.0 && bits(d.s1[1]) == bits(0.0));
    std::vector<float> counts((size_t)m), o0((size_t)m), o1((size_t)m), o2((size_t)m);
    const float* in = v.data(); float* outs[3] = { o0.data(), o1.data(), o2.data() };
    int64_t ungrouped = -1;
    group_sums_host(index.data(), (int64_t)index.size(), m, &in, 1, 7u, counts.data(), outs, &ungrouped);
    CHECK(ungrouped == 8 && counts[1] == 0.0f && bits(o0[1]) == bits(0.0f) && bits(o1[1]) == FM_SELECT_NAN_BITS && bits(o2[1]) == FM_SELECT_NAN_BITS);
    CHECK(o0[3] == 22.0f && o1[3] == 11.0f && o2[3] == 1.0f && o1[0] == 8.5f && o2[0] == 0.25f);
    // every element ungrouped; counts only
    const std::vector<float> none{ nan, -1.0f, 7.0f };
    group_sums_host(none.data(), 3, m, nullptr, 0, 0u, counts.data(), nullptr, &ungrouped);
    CHECK(ungrouped == 3 && counts[0] == 0.0f && counts[3] == 0.0f);
    CHECK(group_sort_passes(1) == 1 && group_sort_passes(255) == 1 && group_sort_passes(256) == 2 && group_sort_passes(65535) == 2 && group_sort_passes(65536) == 3 && group_sort_passes(FM_GROUP_MAX_M - 1) == 3 && group_sort_passes(FM_GROUP_MAX_M) == 4);
    for (int64_t m : { int64_t(1), int64_t(255), int64_t(256), int64_t(65535), int64_t(65536), FM_GROUP_MAX_M - 1, FM_GROUP_MAX_M }) CHECK((uint64_t)m >> (8 * group_sort_passes(m)) == 0);      // every key 0 … m is ordered whole
    CHECK(group_key(nan, 4) == 4u && group_key(-0.0f, 4) == 0u && group_key(3.0f, 4) == 3u && group_key(4.0f, 4) == 4u);
}

static void complaints() {
    const float index[3] = { 0, 1, 2 }, v[3] = { 1, 2, 3 };
    const float* in[5] = { v, v, v, v, v }; const float* holed[1] = { nullptr };
    float c[3], o[3]; float* outs[1] = { o }; float* no_outs[1] = { nullptr };
    int64_t u;
    refused([&] { group_sums_host(index, 3, 0, in, 1, 1u, c, outs, &u); }, "m = 0");
    refused([&] { group_sums_host(index, 3, FM_GROUP_MAX_M + 1, in, 1, 1u, c, outs, &u); }, "m above 2^24");
    refused([&] { group_sums_host(index, 3, 3, in, -1, 1u, c, outs, &u); }, "n_values = -1");
    refused([&] { group_sums_host(index, 3, 3, in, 5, 1u, c, outs, &u); }, "n_values = 5");
    refused([&] { group_sums_host(index, 3, 3, in, 1, 0u, c, outs, &u); }, "a mask of 0 with a value vector");
    refused([&] { group_sums_host(index, 3, 3, in, 1, 8u, c, outs, &u); }, "a mask with unknown bits");
    refused([&] { group_sums_host(index, 3, 3, nullptr, 0, 0u, nullptr, nullptr, nullptr); }, "nothing asked for");
    refused([&] { group_sums_host(index, 0, 3, in, 1, 1u, c, outs, &u); }, "n = 0");
    refused([&] { group_sums_host(index, int64_t(1) << 31, 3, in, 1, 1u, c, outs, &u); }, "n = 2^31");
    refused([&] { group_sums_host(nullptr, 3, 3, in, 1, 1u, c, outs, &u); }, "index null");
    refused([&] { group_sums_host(index, 3, 3, nullptr, 1, 1u, c, outs, &u); }, "values null");
    refused([&] { group_sums_host(index, 3, 3, holed, 1, 1u, c, outs, &u); }, "values[0] null");
    refused([&] { group_sums_host(index, 3, 3, in, 1, 1u, c, nullptr, &u); }, "outs null");
    refused([&] { group_sums_host(index, 3, 3, in, 1, 1u, c, no_outs, &u); }, "outs[0] null");
}

int main() {
    std::mt19937 rng(20261021u);
    one_group_is_the_prefix_total(rng);
    single_members_and_minus_zero();
    the_bound_and_independence(rng);
    membership_and_the_empty_group();
    complaints();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("group host ok\n");
    return 0;
}
