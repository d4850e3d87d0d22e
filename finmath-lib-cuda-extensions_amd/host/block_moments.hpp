// block_moments.hpp — the DEFINITION of the block moments (contract: include/fmhip.h; kernels: csrc/nested_kernel.hip;
// engine side: csrc/nested_engine.hpp).  One header that the host and hipcc both compile: + − × / and comparisons in fp64, no library call,
// no contraction (-ffp-contract=off in every build that includes it).
//
// A vector of n = m·block elements is m consecutive blocks of `block` elements.  For block q, S1[q] is the fp64 sum of (double)v[q·block + i]
// and S2[q] the fp64 sum of the exact fp64 squares (double)x·(double)x (a float's square has at most 48 significant bits), i < block.
//
// THE ASSOCIATION is a function of `block` ALONE — not of q, m, the number of vectors of a call, a vector's slot, the output mask or the
// slicing of a launch.  Both sums are made in the same nested units, each a sum over 64 LEAVES:
//   level 0  a term: the element, or its square.
//   level 1  a segment = FM_BLOCK_SEGMENT (2048) consecutive terms of the block (the last one as far as the block goes).  Leaf l of a
//            segment is the running sum of its terms l, l + 64, l + 128, … in that order, the first term taken as it is; the segment's sum
//            is the butterfly over the 64 leaves (below).  A block of at most 2048 elements is ONE segment and ends here.
//   level 2  a longer block: its ceil(block / 2048) segment sums are the terms of one more unit of the same shape — leaf l is the running
//            sum of the segment sums l, l + 64, …, and the block's sum is the butterfly over those 64 leaves.
// The butterfly: six rounds over the leaf index, bit 5 first — s[l] = s[l] + s[l ^ 32] for every l, then ^ 16, 8, 4, 2, 1 — and the sum is
// s[0] (every s[l] holds the same bits: fl(a + b) = fl(b + a)).  As a recursion: R(l, 64) = leaf l, R(l, s) = R(l, 2s) + R(l + s, 2s), sum =
// R(0, 1).  A leaf WITHOUT a term is −0.0: fl(x + (−0.0)) = x bit for bit for every x that is no NaN (−0.0 + (−0.0) = −0.0 too), so a unit
// of w <= 64 terms has the bits of the butterfly of width w' = the power of two >= w over those terms alone — rounds whose partner index is
// >= w' add −0.0 — which is what lets several small blocks share one wave on the device, each in w' lanes, and fm_block_sums below stop at w'.
// A block of one element is that element; a block of −0.0 alone sums to −0.0.
//
// THE BOUND.  The longest chain of additions behind a sum is fm_block_chain(block) = (ceil(min(block, 2048) / 64) − 1) + 6, plus for a block
// above 2048 elements (ceil(segments / 64) − 1) + 6 with segments = ceil(block / 2048); with exact terms
//     |S − exact| <= (fm_block_chain(block) + 1)·2⁻⁵³·Σ|terms|                 (first order in 2⁻⁵³; the + 1 covers the squares' rounding: none)
// tests/test_nested_cpu.py and tests/cpp/test_block_moments_host.cpp hold the definition to it against an exact sum.
//
// THE OUTPUTS of a block, each rounded to fp32 ONCE from fp64:  sum (float)S1;  mean (float)(S1 / block);  variance
// (float)max(0, S2/block − (S1/block)²), the population variance from RAW fp64 moments: its absolute error is about
// fm_block_chain(block)·2⁻⁵³·S2/block — adequate for the standard error of an inner estimate of a nested simulation, NOT a replacement for
// the shifted pass behind getVariance (a block whose mean is 10⁸ standard deviations has no correct bit here).  NaN and ±∞ propagate as fp64
// arithmetic propagates them (a block with +∞ has sum and mean +∞ and a NaN variance); of a NaN only that it is one is promised (the outputs
// carry the canonical one, 0x7fc00000).  Other blocks are untouched.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define FM_BLOCK_HD __host__ __device__
#else
#define FM_BLOCK_HD
#endif

namespace fmhost {

constexpr int FM_BLOCK_SUM = 1, FM_BLOCK_MEAN = 2, FM_BLOCK_VARIANCE = 4;         // FMHIP_BLOCK_*: the output mask, ascending bit order
constexpr int FM_BLOCK_ALL = 7;
constexpr int FM_BLOCK_MAX_VECTORS = 4;                                            // input vectors of one call
constexpr int FM_BLOCK_MAX_OUTPUTS = 3;
constexpr int FM_BLOCK_LEAVES = 64;                                                // leaves of a unit: the lanes of a wave
constexpr int64_t FM_BLOCK_SEGMENT = 2048;                                         // terms of a segment: 32 per leaf
constexpr int64_t FM_BLOCK_MAX_N = 0x7fffffffLL;                                   // elements of a vector of a call, of the output of a repeat

FM_BLOCK_HD inline int fm_block_outputs(uint32_t mask) { return (int)((mask & 1u) + ((mask >> 1) & 1u) + ((mask >> 2) & 1u)); }
FM_BLOCK_HD inline int64_t fm_block_segments(int64_t block) { return (block + FM_BLOCK_SEGMENT - 1) / FM_BLOCK_SEGMENT; }
// the lanes a unit of `terms` (1 … 64) terms needs: the power of two >= terms
FM_BLOCK_HD inline int fm_block_width(int64_t terms) { int w = 1; while (w < terms) w <<= 1; return w; }
// the longest chain of additions behind a block's sum
FM_BLOCK_HD inline int64_t fm_block_chain(int64_t block)
{
    const int64_t first = block < FM_BLOCK_SEGMENT ? block : FM_BLOCK_SEGMENT;
    int64_t chain = (first + FM_BLOCK_LEAVES - 1) / FM_BLOCK_LEAVES - 1 + 6;
    if (block > FM_BLOCK_SEGMENT) chain += (fm_block_segments(block) + FM_BLOCK_LEAVES - 1) / FM_BLOCK_LEAVES - 1 + 6;
    return chain;
}

struct BlockSums { double s1, s2; };

FM_BLOCK_HD inline float fm_block_narrow(double r)
{
    if (r != r) { const uint32_t b = 0x7fc00000u; float f; __builtin_memcpy(&f, &b, 4); return f; }
    return (float)r;
}
// output j of the mask's bit `bit` from a block's sums
FM_BLOCK_HD inline float fm_block_output(int bit, BlockSums s, int64_t block)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (bit == FM_BLOCK_SUM) return fm_block_narrow(s.s1);
    const double b = (double)block, mean = s.s1 / b;
    if (bit == FM_BLOCK_MEAN) return fm_block_narrow(mean);
    const double d = s.s2 / b - mean * mean;
    return fm_block_narrow(d < 0.0 ? 0.0 : d);                                      // (a NaN is not below 0: it stays)
}

// One unit: `count` >= 1 terms, term k = s1[k·stride], s2[k·stride] — leaves, then the butterfly at the width the terms need.
FM_BLOCK_HD inline BlockSums fm_block_unit(const double* s1, const double* s2, int64_t count, int64_t stride)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double a[FM_BLOCK_LEAVES], b[FM_BLOCK_LEAVES];
    const int w = fm_block_width(count < FM_BLOCK_LEAVES ? count : FM_BLOCK_LEAVES);
    for (int l = 0; l < w; ++l) {
        if (l >= count) { a[l] = -0.0; b[l] = -0.0; continue; }
        double x = s1[(int64_t)l * stride], y = s2[(int64_t)l * stride];
        for (int64_t k = l + FM_BLOCK_LEAVES; k < count; k += FM_BLOCK_LEAVES) { x = x + s1[k * stride]; y = y + s2[k * stride]; }
        a[l] = x; b[l] = y;
    }
    for (int off = w >> 1; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) { a[l] = a[l] + a[l + off]; b[l] = b[l] + b[l + off]; }
    BlockSums r; r.s1 = a[0]; r.s2 = b[0];
    return r;
}

// A segment of the block: `count` (1 … 2048) consecutive elements.
FM_BLOCK_HD inline BlockSums fm_block_segment(const float* v, int64_t count)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double a[FM_BLOCK_LEAVES], b[FM_BLOCK_LEAVES];
    const int w = fm_block_width(count < FM_BLOCK_LEAVES ? count : FM_BLOCK_LEAVES);
    for (int l = 0; l < w; ++l) {
        if (l >= count) { a[l] = -0.0; b[l] = -0.0; continue; }
        double x = (double)v[l], y = x * x;
        for (int64_t k = l + FM_BLOCK_LEAVES; k < count; k += FM_BLOCK_LEAVES) { const double t = (double)v[k]; x = x + t; y = y + t * t; }
        a[l] = x; b[l] = y;
    }
    for (int off = w >> 1; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) { a[l] = a[l] + a[l + off]; b[l] = b[l] + b[l + off]; }
    BlockSums r; r.s1 = a[0]; r.s2 = b[0];
    return r;
}

} // namespace fmhost

#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

// what can be said about a call without looking at a vector
inline void blockCheckMask(uint32_t mask)
{
    if (mask == 0u || (mask & ~(uint32_t)FM_BLOCK_ALL) != 0u) throw std::invalid_argument("block moments: mask " + std::to_string(mask) + " (FMHIP_BLOCK_SUM | FMHIP_BLOCK_MEAN | FMHIP_BLOCK_VARIANCE, at least one)");
}
inline void blockCheckShape(int64_t n, int64_t block)
{
    if (block < 1) throw std::invalid_argument("block moments: blocks of " + std::to_string(block) + " elements (at least 1)");
    if (n < 1 || n > FM_BLOCK_MAX_N) throw std::invalid_argument("block moments of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    if (n % block != 0) throw std::invalid_argument("block moments: " + std::to_string(n) + " elements are no whole number of blocks of " + std::to_string(block));
}
inline void repeatCheck(int64_t n, int64_t each, int64_t times)
{
    if (each < 1 || times < 1) throw std::invalid_argument("repeat: each = " + std::to_string(each) + ", times = " + std::to_string(times) + " (both at least 1)");
    if (n < 1) throw std::invalid_argument("repeat of an empty vector");
    if (each > FM_BLOCK_MAX_N / n || times > FM_BLOCK_MAX_N / (n * each)) throw std::invalid_argument("repeat: an output of " + std::to_string(n) + " x " + std::to_string(each) + " x " + std::to_string(times) + " elements: at most 2^31 - 1");
}

// The sums of ONE block.
inline BlockSums fm_block_sums(const float* v, int64_t block)
{
    if (block <= FM_BLOCK_SEGMENT) return fm_block_segment(v, block);
    const int64_t segments = fm_block_segments(block);
    std::vector<double> s1((size_t)segments), s2((size_t)segments);
    for (int64_t s = 0; s < segments; ++s) {
        const int64_t e0 = s * FM_BLOCK_SEGMENT, cnt = block - e0 < FM_BLOCK_SEGMENT ? block - e0 : FM_BLOCK_SEGMENT;
        const BlockSums p = fm_block_segment(v + e0, cnt);
        s1[(size_t)s] = p.s1; s2[(size_t)s] = p.s2;
    }
    return fm_block_unit(s1.data(), s2.data(), segments, 1);
}

// fmhip_block_moments_host: outs[j·m + q], m = n / block, j over the mask's bits in ascending order.
inline void block_moments_host(const float* v, int64_t n, int64_t block, uint32_t mask, float* outs)
{
    if (!v || !outs) throw std::invalid_argument("block moments: null pointer");
    blockCheckMask(mask);
    blockCheckShape(n, block);
    const int64_t m = n / block;
    for (int64_t q = 0; q < m; ++q) {
        const BlockSums s = fm_block_sums(v + q * block, block);
        int j = 0;
        for (int bit = 1; bit <= FM_BLOCK_VARIANCE; bit <<= 1)
            if (mask & (uint32_t)bit) outs[(int64_t)(j++) * m + q] = fm_block_output(bit, s, block);
    }
}

// the repeat's definition: out[(t·n + p)·each + e] = v[p], bit for bit
inline void repeat_host(const float* v, int64_t n, int64_t each, int64_t times, float* out)
{
    if (!v || !out) throw std::invalid_argument("repeat: null pointer");
    repeatCheck(n, each, times);
    for (int64_t t = 0; t < times; ++t)
        for (int64_t p = 0; p < n; ++p)
            for (int64_t e = 0; e < each; ++e) __builtin_memcpy(&out[(t * n + p) * each + e], &v[p], 4);
}

} // namespace fmhost
#endif
