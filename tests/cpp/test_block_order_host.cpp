// test_block_order_host.cpp — the host half of the block order statistics (host/block_order.hpp) as a stand-alone program, built with
// AddressSanitizer + UBSan by tests/test_block_order_cpu.py: the definition against a plain sort with the comparison of
// java.util.Arrays.sort(float[]) written out, a range sum against a long-double sum within its bound, its independence of where a block
// sits and of the other selectors, the special values, and every refusal.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>

#include "../../finmath-lib-cuda-extensions_amd/host/block_order.hpp"

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
        switch ((s >> 5) % 23u) {
            case 0: x = 0.f; break;
            case 1: x = -0.f; break;
            case 2: x = of_bits(0x7fc00000u | (s >> 12)); break;                           // NaNs of both signs, many payloads
            case 3: x = of_bits(0xff800001u + (s >> 12)); break;
            case 4: x = 2.5f; break;                                                        // ties
            case 5: x = of_bits(((s >> 9) & 0x007fffffu) | ((s & 64u) << 25)); break;                          // denormals of both signs
            default: break;
        }
        a[(size_t)p] = x;
    }
    return a;
}

static void refused(const char* what, const std::function<void()>& f) {
    try { f(); } catch (const std::invalid_argument&) { return; }
    fail(what, 0, 0);
}

int main() {
    // the key and its inverse
    for (uint32_t u : { 0u, 0x80000000u, 1u, 0x80000001u, 0x7f800000u, 0xff800000u, 0x3f800000u, 0xbf800000u, 0x007fffffu })
        if (fm_order_bits(fm_order_key(u)) != u) fail("the key does not come back", u, 0);
    for (uint32_t u : { 0x7fc00000u, 0x7f800001u, 0xffc00000u, 0xffffffffu })
        if (fm_order_key(u) != FM_ORDER_NAN_KEY || fm_order_bits(fm_order_key(u)) != FM_ORDER_NAN_BITS) fail("a NaN's key", u, 0);
    if (!(fm_order_key(0xff800000u) < fm_order_key(0x80000001u) && fm_order_key(0x80000000u) < fm_order_key(0u) && fm_order_key(0x7f800000u) < FM_ORDER_NAN_KEY)) fail("the key's order", 0, 0);

    for (int64_t block : { 1, 2, 3, 63, 64, 65, 128, 129, 1000, 2048, 2049, 4096 }) {
        const int64_t m = block < 100 ? 9 : 3, n = m * block;
        const std::vector<float> a = data(n, (uint32_t)block);
        const int64_t ranks[5] = { 0, block - 1, block / 2, block / 100, 0 };
        const int64_t from[4] = { 0, 0, 0, block / 2 }, to[4] = { 0, block - 1, block / 20, block - 1 };
        std::vector<float> got((size_t)(9 * m), -1.f), sorted((size_t)n, -1.f);
        block_order_statistics_host(a.data(), n, block, ranks, 5, from, to, 4, got.data());
        block_sort_host(a.data(), n, block, sorted.data());
        for (int64_t q = 0; q < m; ++q) {
            std::vector<float> s(a.begin() + q * block, a.begin() + (q + 1) * block);
            std::stable_sort(s.begin(), s.end(), java_less);
            for (float& x : s) if (x != x) x = of_bits(FM_ORDER_NAN_BITS);
            for (int64_t i = 0; i < block; ++i) if (bits_of(sorted[(size_t)(q * block + i)]) != bits_of(s[(size_t)i])) fail("block sort", block, q * block + i);
            for (int j = 0; j < 5; ++j) if (bits_of(got[(size_t)(j * m + q)]) != bits_of(s[(size_t)ranks[j]])) fail("a rank", block, j);
            for (int j = 0; j < 4; ++j) {
                const int64_t count = to[j] - from[j] + 1;
                const float g = got[(size_t)((5 + j) * m + q)];
                long double exact = 0.0L, magnitude = 0.0L; bool nan = false, plus = false, minus = false;
                for (int64_t i = from[j]; i <= to[j]; ++i) {
                    const float x = s[(size_t)i];
                    nan |= x != x; plus |= x == std::numeric_limits<float>::infinity(); minus |= x == -std::numeric_limits<float>::infinity();
                    if (std::isfinite(x)) { exact += (long double)x; magnitude += std::fabs((long double)x); }
                }
                if (nan || (plus && minus)) { if (bits_of(g) != FM_ORDER_NAN_BITS) fail("a range with a NaN or both infinities is the quiet NaN", block, j); continue; }
                if (plus || minus) { if (g != (plus ? 1.f : -1.f) * std::numeric_limits<float>::infinity()) fail("a range with an infinity", block, j); continue; }
                // the definition's sum, by its own pieces, then the bound against the exact sum (the long-double sum of <= 4096 floats is exact to 2^-64 relative)
                const double S = fm_block_sums(s.data() + from[j], count).s1;
                if (bits_of(g) != bits_of(fm_order_mean(S, count))) fail("a range mean is not the mean of fm_block_sums", block, j);
                const long double bound = (long double)(fm_block_chain(count) + 1) * std::ldexp(1.0L, -53) * magnitude + std::ldexp(1.0L, -60) * magnitude;
                if (std::fabs((long double)S - exact) > bound) fail("a range sum is outside its bound", block, j);
            }
        }
        // one selector at a time, and the block among others: the same bits
        for (int j = 0; j < 4; ++j) {
            std::vector<float> alone((size_t)m, -1.f);
            block_order_statistics_host(a.data(), n, block, nullptr, 0, from + j, to + j, 1, alone.data());
            for (int64_t q = 0; q < m; ++q) if (bits_of(alone[(size_t)q]) != bits_of(got[(size_t)((5 + j) * m + q)])) fail("a range depends on the other selectors", block, j);
        }
        std::vector<float> one(a.begin() + block, a.begin() + 2 * block), first(9, -1.f);
        std::reverse(one.begin(), one.end());
        block_order_statistics_host(one.data(), block, block, ranks, 5, from, to, 4, first.data());
        for (int j = 0; j < 9; ++j) if (bits_of(first[(size_t)j]) != bits_of(got[(size_t)(j * m + 1)])) fail("a block depends on where it sits or on its order", block, j);
    }
    {   // in place, and the refusals
        float a[6] = { 3.f, 1.f, 2.f, -0.f, 0.f, -1.f }, out[6];
        block_sort_host(a, 6, 3, a);
        const float want[6] = { 1.f, 2.f, 3.f, -1.f, -0.f, 0.f };
        for (int i = 0; i < 6; ++i) if (bits_of(a[i]) != bits_of(want[i])) fail("block sort in place", i, 0);
        const int64_t r[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }, lo[5] = { 0, 0, 0, 0, 0 }, hi[5] = { 1, 1, 1, 1, 1 }, three[1] = { 3 }, minus[1] = { -1 }, two[1] = { 2 };
        refused("no selector", [&] { block_order_statistics_host(a, 6, 3, r, 0, lo, hi, 0, out); });
        refused("nine ranks", [&] { block_order_statistics_host(a, 6, 3, r, 9, lo, hi, 0, out); });
        refused("five ranges", [&] { block_order_statistics_host(a, 6, 3, r, 0, lo, hi, 5, out); });
        refused("a negative count", [&] { block_order_statistics_host(a, 6, 3, r, -1, lo, hi, 1, out); });
        refused("a rank outside", [&] { block_order_statistics_host(a, 6, 3, three, 1, lo, hi, 0, out); });
        refused("a negative rank", [&] { block_order_statistics_host(a, 6, 3, minus, 1, lo, hi, 0, out); });
        refused("a range outside", [&] { block_order_statistics_host(a, 6, 3, r, 0, lo, three, 1, out); });
        refused("from > to", [&] { block_order_statistics_host(a, 6, 3, r, 0, two, hi, 1, out); });
        refused("block 0", [&] { block_order_statistics_host(a, 6, 0, r, 1, lo, hi, 0, out); });
        refused("no whole number of blocks", [&] { block_order_statistics_host(a, 6, 4, r, 1, lo, hi, 0, out); });
        refused("empty", [&] { block_order_statistics_host(a, 0, 1, r, 1, lo, hi, 0, out); });
        refused("null", [&] { block_order_statistics_host(nullptr, 6, 3, r, 1, lo, hi, 0, out); });
        refused("null ranks", [&] { block_order_statistics_host(a, 6, 3, nullptr, 1, lo, hi, 0, out); });
        refused("sort: block 0", [&] { block_sort_host(a, 6, 0, out); });
        refused("sort: no whole number of blocks", [&] { block_sort_host(a, 6, 4, out); });
        refused("sort: null", [&] { block_sort_host(a, 6, 3, nullptr); });
        if (!blockOrderTooLong(4097) || blockOrderTooLong(4096)) fail("the longest block", 0, 0);
    }
    std::printf("block order host ok\n");
    return 0;
}
