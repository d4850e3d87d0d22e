// test_cross_order_host.cpp — the host half of the order statistics across vectors (host/cross_order.hpp) as a stand-alone program, built
// with AddressSanitizer + UBSan by tests/test_cross_order_cpu.py: the definition against a plain stable sort with the comparison of
// java.util.Arrays.sort(float[]) written out, for every K of the issue's list and sizes around a wave; the compare-exchange network of
// every padded size against the same sort (pairs and keys alone, with the pads the kernels use); the multiset and permutation
// properties; the selection behind an index and behind every index that names no slot; and every refusal.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "../../finmath-lib-cuda-extensions_amd/host/cross_order.hpp"

using namespace fmhost;

static void fail(const char* what, long long a, long long b) { std::fprintf(stderr, "%s (%lld, %lld)\n", what, a, b); std::exit(1); }
static uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static float of_bits(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

// Float.compare: −0.0 < +0.0, every NaN equal and above everything
static bool java_less(float a, float b) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return !na && nb;
    if (a < b) return true;
    if (a > b) return false;
    return (bits_of(a) >> 31) > (bits_of(b) >> 31);
}

static std::vector<float> data(int64_t n, uint32_t seed) {
    std::vector<float> a((size_t)n);
    uint32_t s = seed * 2654435761u + 7u;
    for (int64_t p = 0; p < n; ++p) {
        s = s * 1664525u + 1013904223u;
        float x = std::ldexp((float)(1 + (s >> 20)), (int)((s >> 8) % 53u) - 38);
        if (s & 16u) x = -x;
        switch ((s >> 5) % 13u) {
            case 0: x = 0.f; break;
            case 1: x = -0.f; break;
            case 2: x = of_bits(0x7fc00000u | (s >> 12)); break;                           // NaNs of both signs, many payloads
            case 3: x = of_bits(0xff800001u | (s >> 12)); break;
            case 4: x = (s & 64u) ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity(); break;
            case 5: x = of_bits((s >> 9) & 0x807fffffu); break;                            // denormals of both signs
            case 6: x = (float)(p % 3); break;                                             // ties across slots: a function of the path alone
            default: break;
        }
        a[(size_t)p] = x;
    }
    return a;
}

template <int P>
static void check_network(uint32_t seed) {
    for (int K = P / 2 + (P == 2 ? 0 : 1); K <= P; ++K) {
        if (K < 1) continue;
        const std::vector<float> x = data(K, seed + (uint32_t)K);
        uint64_t pairs[P], want[P]; uint32_t keys[P];
        for (int i = 0; i < P; ++i) {
            const uint32_t key = i < K ? fm_order_key(bits_of(x[(size_t)i])) : FM_ORDER_NAN_KEY;
            pairs[i] = want[i] = fm_cross_pair(key, (uint32_t)i); keys[i] = key;
        }
        std::sort(want, want + P);
        fm_cross_network<P>(pairs);
        fm_cross_network<P>(keys);
        for (int i = 0; i < P; ++i) if (pairs[i] != want[i] || keys[i] != fm_cross_pair_key(want[i])) fail("the network is no sort", P, K);
        for (int i = 0; i < K; ++i) if (fm_cross_pair_slot(pairs[i]) >= (uint32_t)K) fail("a pad sorted in front of a real word", P, K);
    }
}

template <class F> static void refused(F&& f, const char* what) {
    try { f(); } catch (const std::invalid_argument&) { return; }
    fail(what, 0, 0);
}

int main() {
    const int Ks[] = { 1, 2, 3, 5, 8, 9, 16, 17, 31, 32 };
    const int64_t ns[] = { 1, 63, 64, 65, 2049 };
    for (int K : Ks) for (int64_t n : ns) {
        std::vector<std::vector<float>> vs;
        for (int i = 0; i < K; ++i) vs.push_back(data(n, (uint32_t)(1000 * K + 7 * i + n)));
        std::vector<const float*> in;
        for (int i = 0; i < K; ++i) in.push_back(vs[(size_t)(i == K - 1 ? 0 : i)].data());             // the same array in the first and the last slot
        std::vector<int> ranks; for (int r = 0; r < K; ++r) ranks.push_back(r);
        std::vector<std::vector<float>> got((size_t)(2 * K), std::vector<float>((size_t)n, -1.f));
        std::vector<float*> out; for (auto& g : got) out.push_back(g.data());
        cross_order_statistics_host(in.data(), K, n, ranks.data(), K, FM_CROSS_ALL, out.data());
        for (int64_t p = 0; p < n; ++p) {
            std::vector<int> order((size_t)K);
            for (int i = 0; i < K; ++i) order[(size_t)i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return java_less(in[(size_t)i][p], in[(size_t)j][p]); });
            uint32_t seen = 0;
            for (int r = 0; r < K; ++r) {
                const float x = in[(size_t)order[(size_t)r]][p];
                const uint32_t want = x != x ? FM_ORDER_NAN_BITS : bits_of(x);
                if (bits_of(got[(size_t)r][(size_t)p]) != want) fail("a value is not the stable sort's", K, p);
                if (got[(size_t)(K + r)][(size_t)p] != (float)order[(size_t)r]) fail("an index is not the stable sort's", K, p);
                seen |= 1u << order[(size_t)r];
            }
            if (seen != (K == 32 ? 0xffffffffu : (1u << K) - 1u)) fail("the indices are no permutation", K, p);
        }
        // a selector's output does not depend on the others or on the mask; duplicates
        const int some[3] = { K - 1, 0, K - 1 };
        std::vector<std::vector<float>> part(3, std::vector<float>((size_t)n, -1.f));
        float* part_out[3] = { part[0].data(), part[1].data(), part[2].data() };
        cross_order_statistics_host(in.data(), K, n, some, 3, FM_CROSS_VALUES, part_out);
        for (int j = 0; j < 3; ++j) if (std::memcmp(part[(size_t)j].data(), got[(size_t)some[j]].data(), (size_t)n * 4) != 0) fail("values depend on the selectors", K, j);
        cross_order_statistics_host(in.data(), K, n, some, 3, FM_CROSS_INDICES, part_out);
        for (int j = 0; j < 3; ++j) if (std::memcmp(part[(size_t)j].data(), got[(size_t)(K + some[j])].data(), (size_t)n * 4) != 0) fail("indices depend on the selectors", K, j);
        // the selection behind the index of rank r is value r wherever that is no NaN
        std::vector<float> picked((size_t)n, -1.f);
        for (int r : { 0, K / 2, K - 1 }) {
            cross_select_host(got[(size_t)(K + r)].data(), in.data(), K, n, picked.data());
            for (int64_t p = 0; p < n; ++p) {
                const uint32_t want = bits_of(got[(size_t)r][(size_t)p]);
                if (want != FM_ORDER_NAN_BITS ? bits_of(picked[(size_t)p]) != want : picked[(size_t)p] == picked[(size_t)p]) fail("the selection is not the value", K, p);
            }
        }
        // indices that name no slot
        const float odd[9] = { -1.f, (float)K, 0.5f, std::nanf(""), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), (float)K - 0.5f, 1e30f, -1e-30f };
        std::vector<float> index((size_t)n);
        for (int64_t p = 0; p < n; ++p) index[(size_t)p] = odd[p % 9];
        cross_select_host(index.data(), in.data(), K, n, picked.data());
        for (int64_t p = 0; p < n; ++p) if (bits_of(picked[(size_t)p]) != FM_ORDER_NAN_BITS) fail("an index that names no slot selected something", K, p);
        for (int64_t p = 0; p < n; ++p) index[(size_t)p] = p % 2 ? (float)(K - 1) : -0.f;
        cross_select_host(index.data(), in.data(), K, n, picked.data());
        for (int64_t p = 0; p < n; ++p) if (bits_of(picked[(size_t)p]) != bits_of(in[(size_t)(p % 2 ? K - 1 : 0)][p])) fail("a selection lost bits (a NaN keeps its payload)", K, p);
    }
    for (uint32_t seed = 1; seed <= 200; ++seed) { check_network<2>(seed); check_network<4>(seed); check_network<8>(seed); check_network<16>(seed); check_network<32>(seed); }
    for (int k = 1; k <= 32; ++k) if (fm_cross_padded(k) < k || fm_cross_padded(k) < 2 || (k > 2 && fm_cross_padded(k) >= 2 * k)) fail("the padded size", k, fm_cross_padded(k));

    // refusals
    const float a[4] = { 1.f, 2.f, 3.f, 4.f };
    float o[4] = { -7.f, -7.f, -7.f, -7.f };
    const float* two[2] = { a, a }; const float* with_null[2] = { a, nullptr };
    std::vector<const float*> many(33, a);
    float* outs[2] = { o, o }; float* out_null[2] = { o, nullptr };
    int r[33] = { 0 }; const int k2[1] = { 2 }, minus[1] = { -1 };
    refused([&] { cross_order_statistics_host(two, 0, 4, r, 1, 1, outs); }, "no vector");
    refused([&] { cross_order_statistics_host(many.data(), 33, 4, r, 1, 1, outs); }, "33 vectors");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 0, 1, outs); }, "no rank");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 33, 1, outs); }, "33 ranks");
    refused([&] { cross_order_statistics_host(two, 2, 4, k2, 1, 1, outs); }, "rank K");
    refused([&] { cross_order_statistics_host(two, 2, 4, minus, 1, 1, outs); }, "rank -1");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 1, 0, outs); }, "mask 0");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 1, 4, outs); }, "mask 4");
    refused([&] { cross_order_statistics_host(two, 2, 0, r, 1, 1, outs); }, "n = 0");
    refused([&] { cross_order_statistics_host(two, 2, int64_t(1) << 31, r, 1, 1, outs); }, "n = 2^31");
    refused([&] { cross_order_statistics_host(nullptr, 2, 4, r, 1, 1, outs); }, "vs null");
    refused([&] { cross_order_statistics_host(two, 2, 4, nullptr, 1, 1, outs); }, "ranks null");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 1, 1, nullptr); }, "outs null");
    refused([&] { cross_order_statistics_host(with_null, 2, 4, r, 1, 1, outs); }, "vs[1] null");
    refused([&] { cross_order_statistics_host(two, 2, 4, r, 1, 3, out_null); }, "outs[1] null");
    refused([&] { cross_select_host(a, two, 0, 4, o); }, "select among none");
    refused([&] { cross_select_host(a, many.data(), 33, 4, o); }, "select among 33");
    refused([&] { cross_select_host(nullptr, two, 2, 4, o); }, "index null");
    refused([&] { cross_select_host(a, nullptr, 2, 4, o); }, "select vs null");
    refused([&] { cross_select_host(a, with_null, 2, 4, o); }, "select vs[1] null");
    refused([&] { cross_select_host(a, two, 2, 4, nullptr); }, "select out null");
    refused([&] { cross_select_host(a, two, 2, 0, o); }, "select n = 0");
    for (float x : o) if (x != -7.f) fail("a refusal wrote", 0, 0);
    std::printf("cross order host ok\n");
    return 0;
}
