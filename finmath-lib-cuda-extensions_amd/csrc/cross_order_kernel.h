// cross_order_kernel.h — host-callable launchers of the kernels of cross_order_kernel.hip (engine side:
// cross_order_engine.hpp; definition: host/cross_order.hpp): selected ranks of the K values of every path, as values and as slots, each a
// new vector; and the element of one of K vectors that a per-path index names.  The grid and the argument checks are functions of the
// sizes alone and live here (no HIP in them: tests/nulldev/null_cross_order.cpp uses them on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/cross_order.hpp"

namespace fm {

constexpr int FM_CROSS_BLOCK = 256;
constexpr int FM_CROSS_MAX_BLOCKS = 2048;              // the grid's cap: above it the grid-stride loop wraps
// paths per lane: 16-byte loads and stores while a lane's words fit in about 64 registers, 8-byte ones up to about 128, 4-byte ones above
// (keys are one register a word, (key, slot) pairs two)
constexpr int cross_paths_per_lane(int padded, bool pairs) { return padded * (pairs ? 2 : 1) <= 16 ? 4 : padded * (pairs ? 2 : 1) <= 32 ? 2 : 1; }

// The selectors arrive ORDERED BY RANK: the outputs that want sorted position r are value_out[value_begin[r] … value_begin[r + 1]) (resp.
// index_out, index_begin), so that the kernel walks the positions with compile-time register indices and stores what each one owes.
struct DevCrossOrderArgs {
    int64_t   n;
    uint32_t  n_vectors, n_values, n_indices, reserved;                  // K; outputs of each kind (0 or the number of selectors)
    uint8_t   value_begin[fmhost::FM_CROSS_MAX_VECTORS + 8], index_begin[fmhost::FM_CROSS_MAX_VECTORS + 8];      // [0 … K] used, non-decreasing, [K] = the count
    uint64_t  v[fmhost::FM_CROSS_MAX_VECTORS];                           // addresses (vectors are padded to 256 B); [K … 31] repeat [K − 1]: the kernel loads every word of its network
    uint64_t  value_out[fmhost::FM_CROSS_MAX_RANKS], index_out[fmhost::FM_CROSS_MAX_RANKS];
};
struct DevCrossSelectArgs {
    int64_t   n;
    uint32_t  n_vectors, reserved;
    uint64_t  index, out;
    uint64_t  v[fmhost::FM_CROSS_MAX_VECTORS];
};

inline uint32_t cross_blocks(int64_t n, int paths_per_lane)
{
    const int64_t per = (int64_t)FM_CROSS_BLOCK * paths_per_lane, tiles = (n + per - 1) / per;
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_CROSS_MAX_BLOCKS ? FM_CROSS_MAX_BLOCKS : tiles);
}
inline bool cross_order_shape_ok(const DevCrossOrderArgs& a)
{
    const uint32_t K = a.n_vectors;
    if (a.n < 1 || a.n > fmhost::FM_CROSS_MAX_N || K < 1 || K > (uint32_t)fmhost::FM_CROSS_MAX_VECTORS) return false;
    if (a.n_values > (uint32_t)fmhost::FM_CROSS_MAX_RANKS || a.n_indices > (uint32_t)fmhost::FM_CROSS_MAX_RANKS || a.n_values + a.n_indices == 0u) return false;
    if (a.value_begin[0] != 0 || a.index_begin[0] != 0 || a.value_begin[K] != a.n_values || a.index_begin[K] != a.n_indices) return false;
    for (uint32_t r = 0; r < K; ++r) if (a.value_begin[r] > a.value_begin[r + 1] || a.index_begin[r] > a.index_begin[r + 1]) return false;
    for (uint32_t i = 0; i < (uint32_t)fmhost::FM_CROSS_MAX_VECTORS; ++i) if (a.v[i] != a.v[i < K ? i : K - 1] || !a.v[i]) return false;
    for (uint32_t o = 0; o < a.n_values; ++o) if (!a.value_out[o]) return false;
    for (uint32_t o = 0; o < a.n_indices; ++o) if (!a.index_out[o]) return false;
    return true;
}
inline bool cross_select_shape_ok(const DevCrossSelectArgs& a)
{
    if (a.n < 1 || a.n > fmhost::FM_CROSS_MAX_N || a.n_vectors < 1 || a.n_vectors > (uint32_t)fmhost::FM_CROSS_MAX_VECTORS || !a.index || !a.out) return false;
    for (uint32_t i = 0; i < a.n_vectors; ++i) if (!a.v[i]) return false;
    return true;
}

hipError_t launch_cross_order(const DevCrossOrderArgs& a, hipStream_t st);
hipError_t launch_cross_select(const DevCrossSelectArgs& a, hipStream_t st);

} // namespace fm
