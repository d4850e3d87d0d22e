// group_host.hpp — the DEFINITION of the device reduce-by-key (fmhip_group_sums_host), compiled by the host AND by the
// kernels (group_kernel.hip): which group an element belongs to is ONE function (select_index of select_host.hpp), the outputs are ONE set
// of formulas (fm_block_output of host/block_moments.hpp) and the sums are made in ONE association, so the device's outputs are the host's
// bit for bit.  fp64 + − × / only, no libm, -ffp-contract=off.  tests/cpp/test_group_host.cpp drives it, sanitized, on the CPU.
//
//   membership    k(j) = select_index(index[j], m): an element whose index is no integer in [0, m − 1] (NaN, ±∞, a fraction, negative, >= m)
//                 belongs to NO group; −0.0 counts as 0.  `ungrouped` is the number of those elements; a bad index is never an error.
//   order         the sorted sequence is all n elements, stably ordered by (k(j) if grouped, else m; j): the members of a group are
//                 consecutive, in ascending path order, and the ungrouped elements are a last run that is never written.  A HEAD is position 0
//                 and every position whose key differs from the one before it.
//   the sums      S1[k] is the fp64 sum of (double)v[j] over the run of k, S2[k] that of the exact squares (double)x·(double)x, both as
//                 RUN-PREFIXES in the tree of prefix_host.hpp (lane 8, group 64, wave 512, tile 2048, chunk, sample: the same constants, the
//                 chunks of the full n) with one addition to its one rule: the first subunit's run-prefixes are taken as they are; subunit
//                 j's base is the last run-prefix of subunit j − 1; an element of subunit j becomes fl(base + its run-prefix inside the
//                 subunit) ONLY if it lies in the run that is open at the subunit's start — if no head lies at or before it inside the
//                 subunit.  Elements at or after the subunit's first head are left as they are.  S[k] is the run-prefix at the run's last
//                 position.
//   outputs       per group, rounded to fp32 once from fp64 (fm_block_narrow: a NaN comes back as 0x7fc00000): count[k] as (float)count
//                 (exact: n of a call with counts <= 2^31 − 1, a count above 2^24 is rounded), the sum (float)S1, the mean (float)(S1 / count),
//                 the variance (float)max(0, S2/count − (S1/count)²) with the caveat host/block_moments.hpp states for it.  An EMPTY group
//                 has count 0, sum +0.0 and NaN for mean and variance.
//
// WHAT FOLLOWS, and what tests/cpp/test_group_host.cpp holds it to:
//   - with one group, the run-prefixes are P of prefix_sums_host bit for bit: S1 is P[n − 1] of fmhip_prefix_sums_host;
//   - a group of one member is that member's value; a lone −0.0 stays −0.0 (nothing is added to 0);
//   - the bits of a group depend on n, the run's start position and its members in path order — NOT on the values of other groups (a base is
//     added only inside the run it came from), not on n_values, a vector's slot or the mask, and not on how a launch is sliced;
//   - |S − exact| <= (prefix_chain(n) + 1)·2⁻⁵³·Σ|members' terms|: relative to the group's OWN terms, not to the sample's — the additions
//     behind a run-prefix are a sub-chain of those behind a prefix of the tree, over the run's terms alone;
//   - a NaN or ±∞ propagates inside its own group only.
#pragma once
#include "select_host.hpp"
#include "../host/block_moments.hpp"

namespace fm {

constexpr int FM_GROUP_MAX_VALUES = 4;
constexpr int64_t FM_GROUP_MAX_M = FM_SELECT_MAX_POSITION_N;          // 2^24: the float index is exact up to here
constexpr uint32_t FM_GROUP_MASK_ALL = (uint32_t)fmhost::FM_BLOCK_ALL;

// the sort key of an element: its group, or m where it belongs to none
FM_SELECT_HD uint32_t group_key(float index, int64_t m)
{
    const int64_t k = select_index(index, m);
    return k < 0 ? (uint32_t)m : (uint32_t)k;
}
// 8-bit radix passes that order keys 0 … m INCLUSIVE (m is the key of an ungrouped element): the bits of m, not of m - 1 — m = 2^24 needs a fourth
constexpr int group_sort_passes(int64_t m) { return m <= 255 ? 1 : m <= 65535 ? 2 : m < (int64_t(1) << 24) ? 3 : 4; }
// output j of the mask's bit `bit` of a group of `count` members (count == 0: +0.0, NaN, NaN)
FM_SELECT_HD float group_output(int bit, double s1, double s2, int64_t count)
{
    fmhost::BlockSums s; s.s1 = s1; s.s2 = s2;
    if (count == 0) { s.s1 = 0.0; s.s2 = 0.0; }
    return fmhost::fm_block_output(bit, s, count);
}

} // namespace fm

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace fm {

// what can be said about the scalars of a call (std::invalid_argument, as the other definitions complain)
inline void group_check_scalars(int64_t m, int n_values, uint32_t mask, bool anything_else_asked)
{
    if (m < 1 || m > FM_GROUP_MAX_M) throw std::invalid_argument("group sums: " + std::to_string(m) + " groups: 1 … 2^24");
    if (n_values < 0 || n_values > FM_GROUP_MAX_VALUES) throw std::invalid_argument("group sums: " + std::to_string(n_values) + " value vectors: 0 … " + std::to_string(FM_GROUP_MAX_VALUES));
    if ((mask & ~FM_GROUP_MASK_ALL) != 0u) throw std::invalid_argument("group sums: mask " + std::to_string(mask) + " (FMHIP_BLOCK_SUM | FMHIP_BLOCK_MEAN | FMHIP_BLOCK_VARIANCE)");
    if (n_values > 0 && mask == 0u) throw std::invalid_argument("group sums: value vectors and a mask of 0");
    if (n_values == 0 && !anything_else_asked) throw std::invalid_argument("group sums: nothing asked for: no value vector, no counts_out and no ungrouped_out");
}
inline void group_check_size(int64_t n)
{
    if (!prefix_size_ok(n)) throw std::invalid_argument("group sums of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
}

// The run-prefixes of ONE unit of `level` (1 … 6) that holds cnt elements, in place: p enters as the terms.  The rule above.
inline void group_unit_host(double* p, const unsigned char* head, int64_t cnt, int level, int64_t chunk_elems)
{
    if (level == 1) {
        for (int64_t i = 1; i < cnt; ++i) if (!head[i]) p[i] = p[i - 1] + p[i];
        return;
    }
    const int64_t sub = level == 2 ? FM_PREFIX_ITEMS : level == 3 ? FM_PREFIX_ITEMS * FM_PREFIX_GROUP : level == 4 ? FM_PREFIX_WAVE_ELEMS : level == 5 ? FM_PREFIX_TILE : chunk_elems;
    for (int64_t off = 0; off < cnt; off += sub) {
        const int64_t c = cnt - off < sub ? cnt - off : sub;
        group_unit_host(p + off, head + off, c, level - 1, chunk_elems);
        if (off > 0) {
            const double base = p[off - 1];
            for (int64_t i = 0; i < c && !head[off + i]; ++i) p[off + i] = base + p[off + i];
        }
    }
}

// The order: perm[r] = the path at sorted position r, key[r] its key (a counting sort: O(n + m)); the number of ungrouped elements comes back.
inline int64_t group_order_host(const float* index, int64_t n, int64_t m, std::vector<uint32_t>& key, std::vector<uint32_t>& perm)
{
    std::vector<int64_t> at((size_t)m + 2, 0);
    std::vector<uint32_t> own((size_t)n);
    for (int64_t j = 0; j < n; ++j) { own[(size_t)j] = group_key(index[j], m); at[(size_t)own[(size_t)j] + 1]++; }
    const int64_t ungrouped = at[(size_t)m + 1];
    for (int64_t k = 0; k <= m; ++k) at[(size_t)k + 1] += at[(size_t)k];
    key.resize((size_t)n); perm.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) { const int64_t r = at[own[(size_t)j]]++; key[(size_t)r] = own[(size_t)j]; perm[(size_t)r] = (uint32_t)j; }
    return ungrouped;
}

// The definition in doubles (the bound test reads it): counts[k], s1[i][k], s2[i][k] for k < m (s1, s2 or any s1[i], s2[i] may be null);
// an empty group has count 0 and sums +0.0.
inline void group_sums_double_host(const float* index, int64_t n, int64_t m, const float* const* values, int n_values, int64_t* counts, double* const* s1, double* const* s2, int64_t* ungrouped_out)
{
    group_check_scalars(m, n_values, n_values > 0 ? FM_GROUP_MASK_ALL : 0u, true);
    group_check_size(n);
    if (!index || (n_values > 0 && !values)) throw std::invalid_argument("group sums: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i]) throw std::invalid_argument("group sums: null pointer");
    std::vector<uint32_t> key, perm;
    const int64_t ungrouped = group_order_host(index, n, m, key, perm);
    if (ungrouped_out) *ungrouped_out = ungrouped;
    std::vector<unsigned char> head((size_t)n);
    for (int64_t r = 0; r < n; ++r) head[(size_t)r] = r == 0 || key[(size_t)r] != key[(size_t)r - 1];
    if (counts) {
        for (int64_t k = 0; k < m; ++k) counts[k] = 0;
        for (int64_t r = 0; r < n; ++r) if (key[(size_t)r] < (uint32_t)m) counts[key[(size_t)r]]++;
    }
    std::vector<double> p((size_t)n);
    for (int i = 0; i < n_values; ++i) {
        for (int square = 0; square < 2; ++square) {
            double* const out = square ? (s2 ? s2[i] : nullptr) : (s1 ? s1[i] : nullptr);
            if (!out) continue;
            for (int64_t r = 0; r < n; ++r) { const double x = (double)values[i][perm[(size_t)r]]; p[(size_t)r] = square ? x * x : x; }
            group_unit_host(p.data(), head.data(), n, 6, prefix_chunk_elems(n));
            for (int64_t k = 0; k < m; ++k) out[k] = 0.0;
            for (int64_t r = 0; r < n; ++r)
                if (key[(size_t)r] < (uint32_t)m && (r == n - 1 || key[(size_t)r + 1] != key[(size_t)r])) out[key[(size_t)r]] = p[(size_t)r];
        }
    }
}

// fmhip_group_sums_host — THE DEFINITION.  counts_out: m floats or null; outs: n_values × popcount(mask) arrays of m floats, vector-major,
// the mask's bits in ascending order; ungrouped_out: or null.
inline void group_sums_host(const float* index, int64_t n, int64_t m, const float* const* values, int n_values, uint32_t mask, float* counts_out, float* const* outs, int64_t* ungrouped_out)
{
    group_check_scalars(m, n_values, mask, counts_out != nullptr || ungrouped_out != nullptr);
    group_check_size(n);
    if (!index || (n_values > 0 && (!values || !outs))) throw std::invalid_argument("group sums: null pointer");
    const int per = fmhost::fm_block_outputs(mask);
    for (int i = 0; i < n_values; ++i) {
        if (!values[i]) throw std::invalid_argument("group sums: null pointer");
        for (int j = 0; j < per; ++j) if (!outs[i * per + j]) throw std::invalid_argument("group sums: null pointer");
    }
    std::vector<int64_t> counts((size_t)m);
    const bool squares = (mask & (uint32_t)fmhost::FM_BLOCK_VARIANCE) != 0u;
    std::vector<double> a(n_values > 0 ? (size_t)m : 0), b(squares && n_values > 0 ? (size_t)m : 0);
    group_sums_double_host(index, n, m, nullptr, 0, counts.data(), nullptr, nullptr, ungrouped_out);
    if (counts_out) for (int64_t k = 0; k < m; ++k) counts_out[k] = (float)counts[(size_t)k];
    for (int i = 0; i < n_values; ++i) {
        double* const pa = a.data(); double* const pb = squares ? b.data() : nullptr;
        group_sums_double_host(index, n, m, values + i, 1, nullptr, &pa, squares ? &pb : nullptr, nullptr);
        int j = 0;
        for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1) {
            if (!(mask & (uint32_t)bit)) continue;
            float* const out = outs[i * per + j++];
            for (int64_t k = 0; k < m; ++k) out[k] = group_output(bit, a[(size_t)k], squares ? b[(size_t)k] : 0.0, counts[(size_t)k]);
        }
    }
}

} // namespace fm
#endif
