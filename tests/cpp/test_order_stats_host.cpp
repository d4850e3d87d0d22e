// The host half of the device order statistics (csrc/order_stats.hpp) without a device: the key order against a comparison sort by
// java.util.Arrays.sort's rules, and the digit-picking loop against histograms counted here on the CPU.
#include "../../finmath-lib-cuda-extensions_amd/csrc/order_stats.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

using namespace fm::os;

static bool java_less(float a, float b) {          // Float.compare(a, b) < 0
    const bool an = a != a, bn = b != b;
    if (an || bn) return !an && bn;
    if (a == 0.0f && b == 0.0f) return std::signbit(a) && !std::signbit(b);
    return a < b;
}
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

int main() {
    std::mt19937 rng(5);
    std::vector<std::vector<float>> vecs(3);
    const float nan_a = std::nanf(""), special[] = { 0.0f, -0.0f, INFINITY, -INFINITY, nan_a, -nan_a, 1e-45f, -1e-45f, 1.0f, 1.0f, 0.5f };
    std::normal_distribution<float> normal;
    for (int i = 0; i < 5000; ++i) { vecs[0].push_back(normal(rng)); vecs[1].push_back(std::max(normal(rng), 0.0f)); vecs[2].push_back(special[rng() % 11]); }
    // keys order like Float.compare, and come back as the value
    for (const auto& v : vecs) for (size_t i = 0; i + 1 < v.size(); ++i) {
        REQUIRE(java_less(v[i], v[i + 1]) == (key_of(v[i]) < key_of(v[i + 1])));
        const double back = value_of_key(key_of(v[i]));
        REQUIRE((v[i] != v[i]) ? back != back : (back == (double)v[i] && std::signbit(back) == std::signbit(v[i])));
    }
    const int count = (int)vecs.size(), n = (int)vecs[0].size();
    int passes = 0;
    HistPass pass = [&](int S, const uint32_t* slots, uint32_t shift, uint64_t* hist) {
        ++passes;
        for (int k = 0; k < count; ++k) {
            const uint32_t ns = slots[(size_t)k * (1 + S)];
            REQUIRE(ns >= 1 && (int)ns <= S && S <= MAX_SLOTS);
            for (uint32_t s = 0; s < ns; ++s) for (float x : vecs[(size_t)k]) {
                const uint32_t key = key_of(x);
                if (((uint64_t)(key ^ slots[(size_t)k * (1 + S) + 1 + s]) >> (shift + 8)) == 0) hist[((size_t)k * S + s) * BINS + ((key >> shift) & 255u)]++;
            }
        }
    };
    std::vector<int64_t> ranks = { 0, 1, n / 2, n - 2, n - 1, 17, 4000, 2500, 2501, 2502, 33 };      // more than MAX_SLOTS: two rounds
    std::vector<Selected> sel((size_t)count * ranks.size());
    select(pass, count, ranks.data(), (int)ranks.size(), sel.data());
    REQUIRE(passes == 8);
    for (int k = 0; k < count; ++k) {
        std::vector<float> sorted = vecs[(size_t)k];
        std::stable_sort(sorted.begin(), sorted.end(), java_less);
        for (size_t j = 0; j < ranks.size(); ++j) {
            const Selected& s = sel[(size_t)k * ranks.size() + j];
            REQUIRE(s.key == key_of(sorted[(size_t)ranks[j]]));
            int64_t below = 0, not_above = 0;
            for (float x : sorted) { below += key_of(x) < s.key; not_above += key_of(x) <= s.key; }
            REQUIRE(s.below == below && s.not_above == not_above && below <= ranks[j] && ranks[j] < not_above);
        }
        // rank sums from two ends and the sum strictly between
        for (auto range : { std::pair<int64_t, int64_t>{ 0, n - 1 }, { 17, 17 }, { 100, 4000 }, { 2500, 2502 } }) {
            const int64_t r[2] = { range.first, range.second };
            Selected ends[2];
            const std::vector<float>& one = vecs[(size_t)k];
            select([&](int S, const uint32_t* slots, uint32_t shift, uint64_t* hist) {
                (void)S;
                for (uint32_t s = 0; s < slots[0]; ++s) for (float x : one) { const uint32_t key = key_of(x); if (((uint64_t)(key ^ slots[1 + s]) >> (shift + 8)) == 0) hist[(size_t)s * BINS + ((key >> shift) & 255u)]++; }
            }, 1, r, 2, ends);
            double inner = 0.0, want = 0.0;
            for (float x : sorted) if (key_of(x) > ends[0].key && key_of(x) < ends[1].key) inner += (double)x;
            for (int64_t i = r[0]; i <= r[1]; ++i) want += (double)sorted[(size_t)i];
            const double got = rank_sum(ends[0], ends[1], r[0], r[1], inner);
            REQUIRE((want != want) ? got != got : (got == want || std::fabs(got - want) <= 1e-9 * (1.0 + std::fabs(want))));
        }
    }
    std::printf("order statistics host loop ok\n");
    return 0;
}
