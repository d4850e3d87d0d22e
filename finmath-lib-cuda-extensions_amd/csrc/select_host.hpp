// select_host.hpp — the DEFINITION of the device selection (fmhip_compress_host, fmhip_expand_host, fmhip_gather_host),
// compiled by the host AND by the kernels (select_kernel.hip): what is selected, the bits of a lane's eight mask elements and the decoding
// of an index are ONE function each, so the device's outputs are the host's bit for bit.  No HIP beyond the __host__ __device__ marks, no
// libm, and no floating-point sum anywhere: counts are integers.  tests/cpp/test_select_host.cpp drives it, sanitized, on the CPU.
//
//   selected(x)   x >= 0.0f in fp32 — the trigger of FMHIP_OP_CHOOSE: a NaN is not selected, -0.0 is, +inf is.
//   q(r)          the number of selected elements of the mask before r; count = the number of all of them.
//   compress      for the selected r, ascending: values_out[i][q(r)] = values[i][r] bit for bit, positions_out[q(r)] = r.  Outputs of `count`
//                 elements (the host twin: arrays of capacity n of which the first `count` are written).
//   expand        the inverse: values_out[i][r] = values[i][q(r)] where selected(mask[r]), otherwise (float)fill.  Every values[i] has
//                 exactly `count` elements.
//   gather        values_out[i][j] = values[i][k] bit for bit where index[j] is an integer k with 0 <= k <= n - 1 (-0.0 counts as 0, the rule
//                 of fm_cross_select_slot; the comparison is made in double: right for every n); anywhere else — not an integer, out of range,
//                 NaN — the quiet NaN 0x7fc00000.
#pragma once
#include "prefix_host.hpp"

#include <cstring>

#if defined(__HIP__)
#define FM_SELECT_HD __host__ __device__ __forceinline__
#else
#define FM_SELECT_HD inline
#endif

namespace fm {

constexpr int FM_SELECT_MAX_VALUES = 8;
constexpr int64_t FM_SELECT_MAX_POSITION_N = int64_t(1) << 24;         // (float)r is exact up to here
constexpr uint32_t FM_SELECT_NAN_BITS = 0x7fc00000u;

FM_SELECT_HD bool select_selected(float x) { return x >= 0.0f; }
// the element of `values` that index x asks for, or -1
FM_SELECT_HD int64_t select_index(float x, int64_t n)
{
    const double d = (double)x;
    if (!(d >= 0.0 && d <= (double)(n - 1))) return -1;
    const int64_t k = (int64_t)d;
    return (double)k == d ? k : -1;
}

// what can be said about the scalars of a call (std::invalid_argument, as the other definitions complain)
inline void select_check_values(const char* what, int n_values, int least)
{
    if (n_values < least || n_values > FM_SELECT_MAX_VALUES)
        throw std::invalid_argument(std::string(what) + ": " + std::to_string(n_values) + " value vectors: " + std::to_string(least) + " … " + std::to_string(FM_SELECT_MAX_VALUES));
}
inline void select_check_size(const char* what, int64_t n, bool want_positions)
{
    if (!prefix_size_ok(n)) throw std::invalid_argument(std::string(what) + " of " + std::to_string(n) + " elements: the size is 1 … 2^31 - 1");
    if (want_positions && n > FM_SELECT_MAX_POSITION_N) throw std::invalid_argument(std::string(what) + ": positions_out is offered up to 2^24 elements, where the float is exact");
}

inline int64_t select_count_host(const float* mask, int64_t n)
{
    int64_t count = 0;
    for (int64_t r = 0; r < n; ++r) count += select_selected(mask[r]) ? 1 : 0;
    return count;
}

// The definitions.  compress: values_out[i] and positions_out have capacity n (either may be null where nothing of that kind is wanted).
inline void compress_host(const float* mask, int64_t n, const float* const* values, int n_values, float* const* values_out, int64_t* positions_out, int64_t* count_out)
{
    select_check_values("compress", n_values, 0);
    select_check_size("compress", n, positions_out != nullptr);
    if (!mask) throw std::invalid_argument("compress: null pointer");
    if (n_values > 0 && (!values || !values_out)) throw std::invalid_argument("compress: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i] || !values_out[i]) throw std::invalid_argument("compress: null pointer");
    int64_t q = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (!select_selected(mask[r])) continue;
        for (int i = 0; i < n_values; ++i) std::memcpy(&values_out[i][q], &values[i][r], 4);
        if (positions_out) positions_out[q] = r;
        ++q;
    }
    if (count_out) *count_out = q;
}

// expand: false (and nothing written) where n_value_elements is not the mask's count — FMHIP_ERR_SIZE_MISMATCH
inline bool expand_host(const float* mask, int64_t n, const float* const* values, int n_values, int64_t n_value_elements, double fill, float* const* values_out)
{
    select_check_values("expand", n_values, 1);
    select_check_size("expand", n, false);
    if (!mask || !values || !values_out) throw std::invalid_argument("expand: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i] || !values_out[i]) throw std::invalid_argument("expand: null pointer");
    if (select_count_host(mask, n) != n_value_elements) return false;
    const float f = (float)fill;
    int64_t q = 0;
    for (int64_t r = 0; r < n; ++r) {
        const bool s = select_selected(mask[r]);
        for (int i = 0; i < n_values; ++i) std::memcpy(&values_out[i][r], s ? &values[i][q] : &f, 4);
        q += s ? 1 : 0;
    }
    return true;
}

// gather: index has m elements, the values n each, the outputs m each
inline void gather_host(const float* index, int64_t m, const float* const* values, int n_values, int64_t n, float* const* values_out)
{
    select_check_values("gather", n_values, 1);
    select_check_size("gather", m, false);
    select_check_size("gather from a vector", n, false);
    if (!index || !values || !values_out) throw std::invalid_argument("gather: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i] || !values_out[i]) throw std::invalid_argument("gather: null pointer");
    for (int64_t j = 0; j < m; ++j) {
        const int64_t k = select_index(index[j], n);
        for (int i = 0; i < n_values; ++i) {
            if (k >= 0) std::memcpy(&values_out[i][j], &values[i][k], 4);
            else std::memcpy(&values_out[i][j], &FM_SELECT_NAN_BITS, 4);
        }
    }
}

} // namespace fm
