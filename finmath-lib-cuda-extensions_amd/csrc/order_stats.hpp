// order_stats.hpp — the HOST half of the device order statistics: the key order, and the loop that turns per-pass digit
// histograms into the key at a rank.  Host-stepped on purpose: whoever can deliver "the histogram of this pass, over the whole sample"
// — one engine, the shards of a device list (histograms added by the front), the ranks of an expectation communicator (one gather per
// pass) — is served by the same loop.  No HIP in this header: tests/cpp/test_order_stats_host.cpp drives it with a histogram made on the CPU.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

namespace fm {
namespace os {

constexpr int BINS = 256;              // 8-bit digits, four passes (kernels.h: FM_OS_BINS)
constexpr int MAX_SLOTS = 8;           // distinct prefixes per vector and pass (kernels.h: FM_OS_MAX_SLOTS); more ranks go in further rounds

// Key of an element: unsigned order of the keys = order of java.util.Arrays.sort(float[]) — -inf < … < -0 < +0 < … < +inf < NaN, every
// NaN (either sign, any payload) the same key.
inline uint32_t key_of_bits(uint32_t u) { return ((u & 0x7fffffffu) > 0x7f800000u) ? 0xffffffffu : ((u >> 31) ? ~u : (u | 0x80000000u)); }
inline uint32_t bits_of_key(uint32_t k) { return k == 0xffffffffu ? 0x7fc00000u : ((k >> 31) ? (k & 0x7fffffffu) : ~k); }
inline uint32_t key_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return key_of_bits(u); }
inline double value_of_key(uint32_t k) { const uint32_t u = bits_of_key(k); float x; std::memcpy(&x, &u, 4); return (double)x; }

// What a pass delivers: for `count` vectors and S slots each — slots[k·(1+S)] = number of prefixes of vector k, then the prefixes — the
// number of elements whose key agrees with the slot's prefix above bit shift+8, by the digit (key >> shift) & 255: hist[(k·S + s)·256 + d].
using HistPass = std::function<void(int S, const uint32_t* slots, uint32_t shift, uint64_t* hist)>;

struct Selected { uint32_t key = 0; int64_t below = 0, not_above = 0; };     // elements with a smaller key / with a key not larger

// out[k·n_ranks + j] = the key at 0-based position ranks[j] of the ascending sample of vector k (every rank in [0, n): the caller checks).
inline void select(const HistPass& pass, int count, const int64_t* ranks, int n_ranks, Selected* out)
{
    for (int j0 = 0; j0 < n_ranks; j0 += MAX_SLOTS) {
        const int R = n_ranks - j0 < MAX_SLOTS ? n_ranks - j0 : MAX_SLOTS;
        std::vector<uint32_t> prefix((size_t)count * R, 0u);
        std::vector<int64_t> below((size_t)count * R, 0), rest((size_t)count * R);
        std::vector<int> slot_of((size_t)count * R, 0);
        for (int k = 0; k < count; ++k) for (int j = 0; j < R; ++j) rest[(size_t)k * R + j] = ranks[j0 + j];
        std::vector<uint32_t> slots;
        std::vector<uint64_t> hist;
        for (uint32_t shift = 24u;; shift -= 8u) {
            // ranks of a vector that still share their prefix share a slot (the first pass: one slot per vector)
            int S = 1;
            std::vector<int> ns((size_t)count, 0);
            for (int k = 0; k < count; ++k) {
                int n_unique = 0;
                for (int j = 0; j < R; ++j) {
                    int s = -1;
                    for (int i = 0; i < j; ++i) if (prefix[(size_t)k * R + i] == prefix[(size_t)k * R + j]) { s = slot_of[(size_t)k * R + i]; break; }
                    slot_of[(size_t)k * R + j] = s >= 0 ? s : n_unique++;
                }
                ns[(size_t)k] = n_unique;
                if (n_unique > S) S = n_unique;
            }
            slots.assign((size_t)count * (1 + S), 0u);
            for (int k = 0; k < count; ++k) {
                slots[(size_t)k * (1 + S)] = (uint32_t)ns[(size_t)k];
                for (int j = 0; j < R; ++j) slots[(size_t)k * (1 + S) + 1 + slot_of[(size_t)k * R + j]] = prefix[(size_t)k * R + j];
            }
            hist.assign((size_t)count * S * BINS, 0ull);
            pass(S, slots.data(), shift, hist.data());
            for (int k = 0; k < count; ++k) for (int j = 0; j < R; ++j) {
                const size_t i = (size_t)k * R + j;
                const uint64_t* h = hist.data() + ((size_t)k * S + slot_of[i]) * BINS;
                int64_t cum = 0;
                int d = 0;
                for (; d < BINS; ++d) { if (cum + (int64_t)h[d] > rest[i]) break; cum += (int64_t)h[d]; }
                if (d == BINS) throw std::runtime_error("order statistics: a pass counted fewer elements than the rank asked for");
                below[i] += cum; rest[i] -= cum; prefix[i] |= (uint32_t)d << shift;
                if (shift == 0u) { Selected& o = out[(size_t)k * n_ranks + j0 + j]; o.key = prefix[i]; o.below = below[i]; o.not_above = below[i] + (int64_t)h[d]; }
            }
            if (shift == 0u) break;
        }
    }
}

// Σ sorted[from..to] from the two selected ends and the fp64 sum of the elements strictly between their keys.  A NaN end gives NaN,
// +inf and -inf both inside give NaN: plain fp64 arithmetic.
inline double rank_sum(const Selected& lo, const Selected& hi, int64_t from, int64_t to, double inner)
{
    if (lo.key == hi.key) return (double)(to - from + 1) * value_of_key(lo.key);
    const int64_t ties_lo = lo.not_above - from, ties_hi = to - hi.below + 1;
    double s = inner;
    if (ties_lo > 0) s = (double)ties_lo * value_of_key(lo.key) + s;
    if (ties_hi > 0) s = s + (double)ties_hi * value_of_key(hi.key);
    return s;
}

} // namespace os
} // namespace fm
