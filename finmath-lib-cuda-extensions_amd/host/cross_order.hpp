// cross_order.hpp — the DEFINITION of the order statistics ACROSS vectors and of the selection behind their index (contract:
// include/fmhip.h; kernels: csrc/cross_order_kernel.hip; engine side: csrc/cross_order_engine.hpp).  One header that the host and hipcc
// both compile, as block_order.hpp is, whose key (fm_order_key / fm_order_bits) it uses.
//
// K vectors v_0 … v_{K−1} of one size n, 1 <= K <= FM_CROSS_MAX_VECTORS; the same array may stand in several slots.  For path p the K pairs
// (fm_order_key(bits of v_i[p]), i) are sorted ascending by key, ties by slot i — the order of java.util.Arrays.sort(float[]) with the
// slots of equal keys in their own order: a STABLE sort, so that the index output is a function of the data alone.
//
//   value of rank r (0 <= r < K)    out[p] = fm_order_bits of the r-th key: an element of the path's K values bit for bit (the sign of a zero,
//                                   a denormal), or the quiet NaN 0x7fc00000 in the NaN tail.
//   index of rank r                 out[p] = the slot of the r-th pair as a float (exact: at most 31).  The slots of all ranks of a path are a
//                                   permutation of 0 … K−1.
// n_ranks = 1 … FM_CROSS_MAX_RANKS selectors, duplicates allowed; a mask chooses values (FM_CROSS_VALUES), indices (FM_CROSS_INDICES) or
// both: the values of all selectors come first, then the indices.  An output depends on the path's K values and on r alone — not on n, the
// other selectors, the mask, the launch, or where the path sits.
//
//   cross_select                    out[p] = v_j[p] bit for bit (a NaN keeps its payload) where idx[p] is an integer j in [0, K) (−0.0 is 0),
//                                   and 0x7fc00000 for every other idx[p]: a fraction, a negative, a value >= K, a NaN, an infinity.  What
//                                   carries a payload behind an index: a weight, a delta, another date's price of the best performer.
//
// The compare-exchange network fm_cross_network<P> (bitonic, every index a compile-time constant) is what the kernels and the null
// device's stand-in sort with; the definition below sorts with std::sort and knows nothing of it.
#pragma once
#include <stdint.h>

#include "block_order.hpp"

namespace fmhost {

constexpr int FM_CROSS_MAX_VECTORS = 32;                                           // K
constexpr int FM_CROSS_MAX_RANKS = 32;                                             // selectors of one call
constexpr int FM_CROSS_VALUES = 1, FM_CROSS_INDICES = 2, FM_CROSS_ALL = 3;         // the output mask
constexpr int64_t FM_CROSS_MAX_N = (int64_t(1) << 31) - 1;

// outputs of a call: n_ranks per set bit of the mask
FM_BLOCK_HD inline int fm_cross_outputs(int n_ranks, int outputs) { return n_ranks * ((outputs & 1) + ((outputs >> 1) & 1)); }
// the network's size: the power of two >= K, at least 2
FM_BLOCK_HD inline int fm_cross_padded(int k) { return k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : k <= 16 ? 16 : 32; }
// (key, slot) as one 64-bit word: its unsigned order is the order of the pairs
FM_BLOCK_HD inline uint64_t fm_cross_pair(uint32_t key, uint32_t slot) { return ((uint64_t)key << 32) | slot; }
FM_BLOCK_HD inline uint32_t fm_cross_pair_key(uint64_t pair) { return (uint32_t)(pair >> 32); }
FM_BLOCK_HD inline uint32_t fm_cross_pair_slot(uint64_t pair) { return (uint32_t)pair; }
FM_BLOCK_HD inline uint32_t fm_cross_pair_key(uint32_t key) { return key; }        // the network on keys alone (no index wanted: equal keys have equal bits)
// the slot an index selects, or −1 (the comparisons are false for a NaN)
FM_BLOCK_HD inline int fm_cross_select_slot(float index, int k)
{
    if (!(index >= 0.0f && index < (float)k)) return -1;
    const int j = (int)index;
    return (float)j == index ? j : -1;
}

// Ascending bitonic network over P = 2^m words held in an array whose every index is a compile-time constant once unrolled: at (k, j) the
// words i and i ^ j are put in order, ascending iff (i & k) == 0.  Distinct words (pairs with distinct slots) have ONE sorted order, so the
// network's result is the stable sort's.
template <int P, class T>
FM_BLOCK_HD inline void fm_cross_network(T (&a)[P])
{
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 2; k <= P; k <<= 1) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = k >> 1; j > 0; j >>= 1) {
#if defined(__clang__)
#pragma unroll
#endif
            for (int i = 0; i < P; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool ascending = (i & k) == 0;
                    const T x = a[i], y = a[l], lo = x < y ? x : y, hi = x < y ? y : x;
                    a[i] = ascending ? lo : hi;
                    a[l] = ascending ? hi : lo;
                }
            }
        }
    }
}

} // namespace fmhost

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>

namespace fmhost {

// what can be said about a call without looking at a vector
inline void crossOrderCheck(int n_vs, const int* ranks, int n_ranks, int outputs)
{
    if (n_vs < 1 || n_vs > FM_CROSS_MAX_VECTORS) throw std::invalid_argument("cross order statistics of " + std::to_string(n_vs) + " vectors: 1 … " + std::to_string(FM_CROSS_MAX_VECTORS));
    if (n_ranks < 1 || n_ranks > FM_CROSS_MAX_RANKS) throw std::invalid_argument("cross order statistics: " + std::to_string(n_ranks) + " ranks (1 … " + std::to_string(FM_CROSS_MAX_RANKS) + ")");
    if (outputs < 1 || outputs > FM_CROSS_ALL) throw std::invalid_argument("cross order statistics: output mask " + std::to_string(outputs) + " (1 values, 2 indices, 3 both)");
    if (!ranks) throw std::invalid_argument("cross order statistics: null pointer: ranks");
    for (int j = 0; j < n_ranks; ++j)
        if (ranks[j] < 0 || ranks[j] >= n_vs) throw std::invalid_argument("cross order statistics: rank " + std::to_string(ranks[j]) + " of " + std::to_string(n_vs) + " vectors");
}
inline void crossSelectCheck(int n_vs)
{
    if (n_vs < 1 || n_vs > FM_CROSS_MAX_VECTORS) throw std::invalid_argument("cross select among " + std::to_string(n_vs) + " vectors: 1 … " + std::to_string(FM_CROSS_MAX_VECTORS));
}
inline void crossCheckSize(int64_t n, const char* what)
{
    if (n < 1 || n > FM_CROSS_MAX_N) throw std::invalid_argument(std::string(what) + " of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
}

// fmhip_cross_order_statistics_host: outs[j] (values, if the mask has them), then outs[n_ranks·(values?) + j] (indices), n floats each
inline void cross_order_statistics_host(const float* const* vs, int n_vs, int64_t n, const int* ranks, int n_ranks, int outputs, float* const* outs)
{
    if (!vs || !outs) throw std::invalid_argument("cross order statistics: null pointer");
    crossOrderCheck(n_vs, ranks, n_ranks, outputs);
    crossCheckSize(n, "cross order statistics");
    const int n_out = fm_cross_outputs(n_ranks, outputs);
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw std::invalid_argument("cross order statistics: vs[" + std::to_string(i) + "] is null");
    for (int o = 0; o < n_out; ++o) if (!outs[o]) throw std::invalid_argument("cross order statistics: outs[" + std::to_string(o) + "] is null");
    float* const* values = (outputs & FM_CROSS_VALUES) ? outs : nullptr;
    float* const* indices = (outputs & FM_CROSS_INDICES) ? outs + (values ? n_ranks : 0) : nullptr;
    uint64_t pairs[FM_CROSS_MAX_VECTORS];
    for (int64_t p = 0; p < n; ++p) {
        for (int i = 0; i < n_vs; ++i) { uint32_t u; __builtin_memcpy(&u, &vs[i][p], 4); pairs[i] = fm_cross_pair(fm_order_key(u), (uint32_t)i); }
        std::sort(pairs, pairs + n_vs);
        for (int j = 0; j < n_ranks; ++j) {
            const uint64_t pair = pairs[ranks[j]];
            if (values) { const uint32_t u = fm_order_bits(fm_cross_pair_key(pair)); __builtin_memcpy(&values[j][p], &u, 4); }
            if (indices) indices[j][p] = (float)fm_cross_pair_slot(pair);
        }
    }
}

// fmhip_cross_select_host
inline void cross_select_host(const float* index, const float* const* vs, int n_vs, int64_t n, float* out)
{
    if (!index || !vs || !out) throw std::invalid_argument("cross select: null pointer");
    crossSelectCheck(n_vs);
    crossCheckSize(n, "cross select");
    for (int i = 0; i < n_vs; ++i) if (!vs[i]) throw std::invalid_argument("cross select: vs[" + std::to_string(i) + "] is null");
    for (int64_t p = 0; p < n; ++p) {
        const int j = fm_cross_select_slot(index[p], n_vs);
        uint32_t u = FM_ORDER_NAN_BITS;
        if (j >= 0) __builtin_memcpy(&u, &vs[j][p], 4);
        __builtin_memcpy(&out[p], &u, 4);
    }
}

} // namespace fmhost
#endif
