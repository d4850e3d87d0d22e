// block_order.hpp — the DEFINITION of the block order statistics and the block sort (contract: include/fmhip.h; kernels:
// csrc/block_order_kernel.hip; engine side: csrc/block_order_engine.hpp).  One header that the host and hipcc both compile, as
// block_moments.hpp is, whose sums (fm_block_sums) and narrowing (fm_block_narrow) it uses: no contraction (-ffp-contract=off).
//
// A vector of n = m·block elements is m consecutive blocks of `block` elements, 1 <= block <= FM_BLOCK_ORDER_MAX.  THE ORDER is that of
// the 32-bit key fm_order_key — csrc/order_stats.hpp's key_of_bits, the order of java.util.Arrays.sort(float[]): −∞ < … < −0.0 < +0.0 < …
// < +∞ < every NaN, all NaNs equal (the key 0xffffffff).  s_q is block q in ascending key order, as 32-bit patterns (fm_order_bits of
// the sorted keys): equal keys have equal bits apart from NaNs, which all come back as the quiet NaN 0x7fc00000 — so s_q, and with it
// everything below, is a function of the block's multiset alone: not of q, m, the other selectors, the vector's slot or the launch.
//
//   rank r (0 <= r < block)             out[q] = s_q[r]: an element of the block bit for bit (its zero's sign, a denormal), or 0x7fc00000 in
//                                       the NaN tail.
//   range mean [from, to]               0 <= from <= to < block, count = to − from + 1.  S = the fp64 sum of s_q[from .. to] in the association
//                                       that fm_block_sums gives an array of `count` elements: leaf l of a segment of 2048 terms is the
//                                       running sum of the terms l, l + 64, … started from −0.0, the butterfly over the 64 leaves with bit 5
//                                       first, and above 2048 terms one more such unit over the (two) segment sums.  out[q] =
//                                       fm_block_narrow(S / count).  A range that reaches the NaN tail, or that holds both infinities, gives
//                                       the quiet NaN.  |S − exact| <= (fm_block_chain(count) + 1)·2⁻⁵³·Σ|terms|.
//   block sort                          out[q·block + i] = s_q[i].  Keys are carried, not (key, index) pairs: fmhip_sort_by_key is the stable,
//                                       payload-preserving sort.
#pragma once
#include <stdint.h>

#include "block_moments.hpp"

namespace fmhost {

constexpr int64_t FM_BLOCK_ORDER_MAX = 4096;                                       // elements of a block
constexpr int FM_BLOCK_ORDER_MAX_VECTORS = 4;                                      // input vectors of one call
constexpr int FM_BLOCK_ORDER_MAX_RANKS = 8, FM_BLOCK_ORDER_MAX_RANGES = 4;         // selectors of one call
constexpr int FM_BLOCK_ORDER_MAX_OUTPUTS = FM_BLOCK_ORDER_MAX_RANKS + FM_BLOCK_ORDER_MAX_RANGES;
constexpr uint32_t FM_ORDER_NAN_KEY = 0xffffffffu, FM_ORDER_NAN_BITS = 0x7fc00000u;

// csrc/order_stats.hpp: key_of_bits / bits_of_key
FM_BLOCK_HD inline uint32_t fm_order_key(uint32_t u) { return ((u & 0x7fffffffu) > 0x7f800000u) ? FM_ORDER_NAN_KEY : ((u >> 31) ? ~u : (u | 0x80000000u)); }
FM_BLOCK_HD inline uint32_t fm_order_bits(uint32_t k) { return k == FM_ORDER_NAN_KEY ? FM_ORDER_NAN_BITS : ((k >> 31) ? (k & 0x7fffffffu) : ~k); }
// the term of a range sum behind a sorted key
FM_BLOCK_HD inline double fm_order_term(uint32_t k) { const uint32_t u = fm_order_bits(k); float x; __builtin_memcpy(&x, &u, 4); return (double)x; }
// the range mean from its sum
FM_BLOCK_HD inline float fm_order_mean(double S, int64_t count)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return fm_block_narrow(S / (double)count);
}

} // namespace fmhost

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>

namespace fmhost {

// what can be said about a call without looking at a vector (a block above FM_BLOCK_ORDER_MAX is not said here: it is UNSUPPORTED, not invalid)
inline void blockOrderCheckBlock(int64_t block, const char* what)
{
    if (block < 1) throw std::invalid_argument(std::string(what) + ": blocks of " + std::to_string(block) + " elements (at least 1)");
}
inline bool blockOrderTooLong(int64_t block) { return block > FM_BLOCK_ORDER_MAX; }
inline std::string blockOrderTooLongWhy(int64_t block, const char* what)
{
    return std::string(what) + ": blocks of " + std::to_string(block) + " elements (at most " + std::to_string(FM_BLOCK_ORDER_MAX) +
           "; fmhip_select_ranks_batch selects in whole vectors, fmhip_sort_by_key sorts them)";
}
inline void blockOrderCheckSelectors(int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to, int n_ranges)
{
    if (n_ranks < 0 || n_ranks > FM_BLOCK_ORDER_MAX_RANKS) throw std::invalid_argument("block order statistics: " + std::to_string(n_ranks) + " ranks (0 … " + std::to_string(FM_BLOCK_ORDER_MAX_RANKS) + ")");
    if (n_ranges < 0 || n_ranges > FM_BLOCK_ORDER_MAX_RANGES) throw std::invalid_argument("block order statistics: " + std::to_string(n_ranges) + " ranges (0 … " + std::to_string(FM_BLOCK_ORDER_MAX_RANGES) + ")");
    if (n_ranks + n_ranges == 0) throw std::invalid_argument("block order statistics: no rank and no range");
    if ((n_ranks > 0 && !ranks) || (n_ranges > 0 && (!range_from || !range_to))) throw std::invalid_argument("block order statistics: null pointer");
    blockOrderCheckBlock(block, "block order statistics");
    for (int j = 0; j < n_ranks; ++j)
        if (ranks[j] < 0 || ranks[j] >= block) throw std::invalid_argument("block order statistics: rank " + std::to_string(ranks[j]) + " of a block of " + std::to_string(block));
    for (int j = 0; j < n_ranges; ++j)
        if (range_from[j] < 0 || range_from[j] > range_to[j] || range_to[j] >= block)
            throw std::invalid_argument("block order statistics: range [" + std::to_string(range_from[j]) + ", " + std::to_string(range_to[j]) + "] of a block of " + std::to_string(block));
}
inline void blockOrderCheckShape(int64_t n, int64_t block, const char* what)
{
    blockOrderCheckBlock(block, what);
    if (n < 1 || n > FM_BLOCK_MAX_N) throw std::invalid_argument(std::string(what) + " of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    if (n % block != 0) throw std::invalid_argument(std::string(what) + ": " + std::to_string(n) + " elements are no whole number of blocks of " + std::to_string(block));
}

// s_q as keys
inline void fm_order_sorted_keys(const float* v, int64_t block, std::vector<uint32_t>& keys)
{
    keys.resize((size_t)block);
    for (int64_t i = 0; i < block; ++i) { uint32_t u; __builtin_memcpy(&u, &v[i], 4); keys[(size_t)i] = fm_order_key(u); }
    std::sort(keys.begin(), keys.end());
}

// fmhip_block_order_statistics_host: outs[j·m + q], m = n / block, ranks first.  A block above FM_BLOCK_ORDER_MAX is defined too (the
// definition has no kernel to fit); the ABI refuses it before it gets here.
inline void block_order_statistics_host(const float* v, int64_t n, int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to,
                                        int n_ranges, float* outs)
{
    if (!v || !outs) throw std::invalid_argument("block order statistics: null pointer");
    blockOrderCheckSelectors(block, ranks, n_ranks, range_from, range_to, n_ranges);
    blockOrderCheckShape(n, block, "block order statistics");
    const int64_t m = n / block;
    std::vector<uint32_t> keys;
    std::vector<float> terms;
    for (int64_t q = 0; q < m; ++q) {
        fm_order_sorted_keys(v + q * block, block, keys);
        for (int j = 0; j < n_ranks; ++j) { const uint32_t u = fm_order_bits(keys[(size_t)ranks[j]]); __builtin_memcpy(&outs[(int64_t)j * m + q], &u, 4); }
        for (int j = 0; j < n_ranges; ++j) {
            const int64_t count = range_to[j] - range_from[j] + 1;
            terms.resize((size_t)count);
            for (int64_t i = 0; i < count; ++i) { const uint32_t u = fm_order_bits(keys[(size_t)(range_from[j] + i)]); __builtin_memcpy(&terms[(size_t)i], &u, 4); }
            outs[(int64_t)(n_ranks + j) * m + q] = fm_order_mean(fm_block_sums(terms.data(), count).s1, count);
        }
    }
}

// fmhip_block_sort_host: out[q·block + i] = s_q[i]
inline void block_sort_host(const float* v, int64_t n, int64_t block, float* out)
{
    if (!v || !out) throw std::invalid_argument("block sort: null pointer");
    blockOrderCheckShape(n, block, "block sort");
    std::vector<uint32_t> keys;
    for (int64_t q = 0; q < n / block; ++q) {
        fm_order_sorted_keys(v + q * block, block, keys);
        for (int64_t i = 0; i < block; ++i) { const uint32_t u = fm_order_bits(keys[(size_t)i]); __builtin_memcpy(&out[q * block + i], &u, 4); }
    }
}

} // namespace fmhost
#endif
