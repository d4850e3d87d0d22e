// tabulated_function.hpp — the definition of a TABULATED FUNCTION applied to every element of a vector (RandomVariable.apply for a curve:
// a local-volatility slice, a Markov-functional numéraire, a payoff profile, an exercise boundary, an inverse empirical CDF), in ONE header
// that the host (g++, hipcc -x c++) and the device (csrc/table_kernel.hip) both compile.  DESIGN.md §4.18; contract: include/fmhip.h.
//
// A table: m knots K[0..m), 1 <= m <= FM_TABLE_MAX_KNOTS, finite and strictly increasing doubles, and for each of T functions (1 <= T <= 4,
// m·T <= 1024) m + 1 SEGMENTS of four fp64 coefficients C[s][0..3].  For an element x (fp32):
//   X = (double)x;  s = the number of knots <= X (0 … m: the last knot belongs to the right end segment);
//   a = K[max(s − 1, 0)], t = X − a;  result = (float)(((C3·t + C2)·t + C1)·t + C0),
// every operation rounded on its own in fp64 (builds: -ffp-contract=off, no fast-math), one final narrowing.  A segment with
// C1 = C2 = C3 = 0 yields (float)C0 for every x in it, the infinite ones included (no 0·∞).  A NaN x — and a result that is a NaN — is the
// quiet NaN 0x7fc00000 on both sides.  Only + − ×, comparisons and integer operations: what the device computes EQUALS what the host does.
//   fm_table_segment_plain     s by a binary search over all knots: the definition
//   fm_table_cell              the cell of X in a uniform grid over [K[0], K[m−1]): the coarse index in front of the search
//   fm_table_segment           s by the index: the cell's range of segments, a binary search inside it, then a correction against K[s−1]
//                              and K[s] — the result is the definition's s for EVERY X and every index whose entries are 0 … m
//   fm_table_value             the polynomial of one segment
// Host only, below: table_index_build (the index), table_build (the coefficients of the interpolation methods), table_apply_host (the
// definition over an array), and their argument checks, which complain with std::invalid_argument.
//
// The interpolation and extrapolation NAMES follow finmath-lib's RationalFunctionInterpolation (InterpolationMethod PIECEWISE_CONSTANT,
// LINEAR, CUBIC_SPLINE, …; ExtrapolationMethod CONSTANT, LINEAR) as remembered, not as read: that class is not part of the reference tree.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define FM_HD __host__ __device__
#else
#define FM_HD
#endif

namespace fmhost {

constexpr int FM_TABLE_MAX_KNOTS = 1024;
constexpr int FM_TABLE_MAX_FUNCTIONS = 4;
constexpr int FM_TABLE_MAX_ENTRIES = 1024;        // knots x functions of one call
constexpr int FM_TABLE_MAX_CELLS = 2048;          // cells of the coarse index; first[] has one entry more
constexpr int FM_TABLE_CELLS_PER_KNOT = 4;

enum { FM_TABLE_PIECEWISE_CONSTANT = 0, FM_TABLE_LINEAR = 1, FM_TABLE_CUBIC_SPLINE = 2, FM_TABLE_MONOTONE_CUBIC = 3 };      // = FMHIP_TABLE_*
enum { FM_TABLE_CONSTANT = 0, FM_TABLE_LINEAR_EXTRAPOLATION = 1 };

FM_HD inline int fm_table_cells(int m) { const int c = FM_TABLE_CELLS_PER_KNOT * m; return c > FM_TABLE_MAX_CELLS ? FM_TABLE_MAX_CELLS : c; }

// the number of knots <= X; 0 for a NaN (whose result does not depend on it)
FM_HD inline int fm_table_segment_plain(const double* K, int m, double X)
{
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (K[mid] <= X) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// K[0] <= X < K[m−1] and 0 <= scale < inf (table_index_build): the product is finite and not negative.  Monotone in X: − and × by a
// non-negative number round monotonically, and so does the truncation.
FM_HD inline int fm_table_cell(double X, double k0, double scale, int cells)
{
    const double u = (X - k0) * scale;
    const int c = (int)u;
    return c < cells - 1 ? c : cells - 1;
}

// k_first = K[0], k_last = K[m − 1]: a caller with many X keeps the two in registers
FM_HD inline int fm_table_segment(const double* K, int m, const uint16_t* first, int cells, double scale, double X, double k_first, double k_last)
{
    if (X != X || X < k_first) return 0;
    if (X >= k_last) return m;
    const int c = fm_table_cell(X, k_first, scale, cells);
    int lo = first[c], hi = first[c + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (K[mid] <= X) lo = mid + 1; else hi = mid;
    }
    while (lo < m && K[lo] <= X) ++lo;              // the index is a hint: these two never run with the index of table_index_build
    while (lo > 0 && K[lo - 1] > X) --lo;
    return lo;
}
FM_HD inline int fm_table_segment(const double* K, int m, const uint16_t* first, int cells, double scale, double X)
{
    return fm_table_segment(K, m, first, cells, scale, X, K[0], K[m - 1]);
}

FM_HD inline float fm_table_qnan() { const uint32_t b = 0x7fc00000u; float f; __builtin_memcpy(&f, &b, 4); return f; }

// c: the four coefficients of X's segment, a: its anchor
FM_HD inline float fm_table_value(const double* c, double X, double a)
{
    if (X != X) return fm_table_qnan();
    const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    if (c1 == 0.0 && c2 == 0.0 && c3 == 0.0) { const float f = (float)c0; return f == f ? f : fm_table_qnan(); }
    const double t = X - a;
    double r = c3 * t;
    r = r + c2;
    r = r * t;
    r = r + c1;
    r = r * t;
    r = r + c0;
    const float f = (float)r;
    return f == f ? f : fm_table_qnan();
}

} // namespace fmhost

#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

inline bool table_finite(double d) { return d - d == 0.0; }

inline void tableCheckKnots(const double* knots, int m)
{
    if (m < 1 || m > FM_TABLE_MAX_KNOTS) throw std::invalid_argument("tabulated function: " + std::to_string(m) + " knots (1 … " + std::to_string(FM_TABLE_MAX_KNOTS) + ")");
    if (!knots) throw std::invalid_argument("tabulated function: null pointer: knots");
    for (int i = 0; i < m; ++i) {
        if (!table_finite(knots[i])) throw std::invalid_argument("tabulated function: knot " + std::to_string(i) + " is not finite");
        if (i > 0 && !(knots[i - 1] < knots[i])) throw std::invalid_argument("tabulated function: the knots are not strictly increasing at " + std::to_string(i));
    }
}

// what fmhip_table_apply and fmhip_table_apply_host can say without looking at a vector
inline void tableCheckApply(const double* knots, int m, const double* coefficients, int n_tables, const void* out)
{
    if (n_tables < 1 || n_tables > FM_TABLE_MAX_FUNCTIONS) throw std::invalid_argument("tabulated function: " + std::to_string(n_tables) + " tables in one call (1 … " + std::to_string(FM_TABLE_MAX_FUNCTIONS) + ")");
    tableCheckKnots(knots, m);
    if ((int64_t)m * n_tables > FM_TABLE_MAX_ENTRIES) throw std::invalid_argument("tabulated function: " + std::to_string(m) + " knots x " + std::to_string(n_tables) + " tables exceed " + std::to_string(FM_TABLE_MAX_ENTRIES));
    if (!coefficients || !out) throw std::invalid_argument("tabulated function: null pointer");
}

// first[c], c = 0 … cells: the number of knots whose cell is below c.  The cell function is monotone, so for an X of cell c the knots of
// lower cells are <= X and those of higher cells are > X: first[c] <= s <= first[c + 1].  The last knot is no X of the grid (X >= K[m−1]
// is the right end segment before the grid is asked) and counts as cell `cells`.  scale = cells / (K[m−1] − K[0]), or 0 where that is not
// finite (m = 1, a range that is denormal): everything is cell 0 then.
inline void table_index_build(const double* K, int m, int cells, double* scale_out, uint16_t* first /* cells + 1 */)
{
    double scale = 0.0;
    if (m > 1) { scale = (double)cells / (K[m - 1] - K[0]); if (!table_finite(scale)) scale = 0.0; }
    for (int c = 0; c <= cells; ++c) first[c] = 0;
    for (int i = 0; i < m; ++i) {
        const int c = i == m - 1 ? cells : fm_table_cell(K[i], K[0], scale, cells);
        if (c < cells) first[c + 1]++;                      // knots of cell c count for every cell above it
    }
    for (int c = 1; c <= cells; ++c) first[c] = (uint16_t)(first[c] + first[c - 1]);
    *scale_out = scale;
}

// coefficients_out[(m + 1) * 4]: segment s = 1 … m − 1 is [K[s−1], K[s]) with anchor K[s−1], segment 0 lies below K[0] (anchor K[0]),
// segment m is [K[m−1], ∞) (anchor K[m−1]).
inline void table_build(const double* knots, const double* values, int m, int interpolation, int extrapolation, int derivative, double* coefficients_out)
{
    tableCheckKnots(knots, m);
    if (!values || !coefficients_out) throw std::invalid_argument("tabulated function: null pointer");
    for (int i = 0; i < m; ++i) if (!table_finite(values[i])) throw std::invalid_argument("tabulated function: value " + std::to_string(i) + " is not finite");
    if (interpolation < FM_TABLE_PIECEWISE_CONSTANT || interpolation > FM_TABLE_MONOTONE_CUBIC) throw std::invalid_argument("tabulated function: interpolation " + std::to_string(interpolation) + " (FMHIP_TABLE_PIECEWISE_CONSTANT … FMHIP_TABLE_MONOTONE_CUBIC)");
    if (extrapolation != FM_TABLE_CONSTANT && extrapolation != FM_TABLE_LINEAR_EXTRAPOLATION) throw std::invalid_argument("tabulated function: extrapolation " + std::to_string(extrapolation) + " (FMHIP_TABLE_CONSTANT or FMHIP_TABLE_LINEAR_EXTRAPOLATION)");
    if (derivative != 0 && derivative != 1) throw std::invalid_argument("tabulated function: derivative " + std::to_string(derivative) + " (0 or 1)");
    const double* K = knots; const double* V = values;
    double* C = coefficients_out;
    for (int i = 0; i < (m + 1) * 4; ++i) C[i] = 0.0;
    int method = interpolation;
    if (m == 1) method = FM_TABLE_PIECEWISE_CONSTANT;
    else if (m < 3 && method >= FM_TABLE_CUBIC_SPLINE) method = FM_TABLE_LINEAR;
    std::vector<double> h((size_t)m), delta((size_t)m);                  // of the interval [K[i], K[i+1]], i < m − 1
    for (int i = 0; i + 1 < m; ++i) { h[(size_t)i] = K[i + 1] - K[i]; delta[(size_t)i] = (V[i + 1] - V[i]) / h[(size_t)i]; }
    double slope_left = 0.0, slope_right = 0.0;                          // of the adjacent segment at the end knots
    for (int i = 0; i < m; ++i) C[(i + 1) * 4] = V[i];
    if (method == FM_TABLE_LINEAR) {
        for (int i = 0; i + 1 < m; ++i) C[(i + 1) * 4 + 1] = delta[(size_t)i];
        slope_left = delta[0]; slope_right = delta[(size_t)m - 2];
    }
    else if (method == FM_TABLE_CUBIC_SPLINE) {
        // natural: M[0] = M[m−1] = 0; h[i−1]·M[i−1] + 2(h[i−1] + h[i])·M[i] + h[i]·M[i+1] = 6(delta[i] − delta[i−1]), by the Thomas algorithm
        std::vector<double> M((size_t)m, 0.0), cp((size_t)m, 0.0), dp((size_t)m, 0.0);
        for (int i = 1; i + 1 < m; ++i) {
            const double lower = i == 1 ? 0.0 : h[(size_t)i - 1], diag = 2.0 * (h[(size_t)i - 1] + h[(size_t)i]), upper = i + 2 == m ? 0.0 : h[(size_t)i];
            const double rhs = 6.0 * (delta[(size_t)i] - delta[(size_t)i - 1]);
            const double den = diag - lower * cp[(size_t)i - 1];
            cp[(size_t)i] = upper / den;
            dp[(size_t)i] = (rhs - lower * dp[(size_t)i - 1]) / den;
        }
        for (int i = m - 2; i >= 1; --i) M[(size_t)i] = dp[(size_t)i] - cp[(size_t)i] * M[(size_t)i + 1];
        for (int i = 0; i + 1 < m; ++i) {
            double* c = C + (i + 1) * 4;
            c[1] = delta[(size_t)i] - h[(size_t)i] * (2.0 * M[(size_t)i] + M[(size_t)i + 1]) / 6.0;
            c[2] = M[(size_t)i] / 2.0;
            c[3] = (M[(size_t)i + 1] - M[(size_t)i]) / (6.0 * h[(size_t)i]);
        }
        slope_left = C[4 + 1];
        slope_right = delta[(size_t)m - 2] + h[(size_t)m - 2] * (2.0 * M[(size_t)m - 1] + M[(size_t)m - 2]) / 6.0;
    }
    else if (method == FM_TABLE_MONOTONE_CUBIC) {
        // Fritsch–Carlson: interior slopes by the weighted harmonic mean of the neighbouring secants (0 where they differ in sign or one is
        // 0), the three-point formula at the ends, limited to keep the shape — PchipInterpolator's definition
        std::vector<double> d((size_t)m, 0.0);
        for (int i = 1; i + 1 < m; ++i) {
            const double d0 = delta[(size_t)i - 1], d1 = delta[(size_t)i];
            if (d0 == d1) d[(size_t)i] = d0;
            else if ((d0 > 0.0 && d1 > 0.0) || (d0 < 0.0 && d1 < 0.0)) {
                const double w1 = 2.0 * h[(size_t)i] + h[(size_t)i - 1], w2 = h[(size_t)i] + 2.0 * h[(size_t)i - 1];
                d[(size_t)i] = (w1 + w2) / (w1 / d0 + w2 / d1);
            }
        }
        auto sign = [](double v) { return v > 0.0 ? 1 : v < 0.0 ? -1 : 0; };
        auto end_slope = [&](double h0, double h1, double d0, double d1) {
            if (d0 == d1) return d0;
            const double e = ((2.0 * h0 + h1) * d0 - h0 * d1) / (h0 + h1);
            if (sign(e) != sign(d0)) return 0.0;
            if (sign(d0) != sign(d1) && (e < 0.0 ? -e : e) > 3.0 * (d0 < 0.0 ? -d0 : d0)) return 3.0 * d0;
            return e;
        };
        d[0] = end_slope(h[0], h[1], delta[0], delta[1]);
        d[(size_t)m - 1] = end_slope(h[(size_t)m - 2], h[(size_t)m - 3], delta[(size_t)m - 2], delta[(size_t)m - 3]);
        for (int i = 0; i + 1 < m; ++i) {
            double* c = C + (i + 1) * 4;
            c[1] = d[(size_t)i];
            c[2] = (3.0 * delta[(size_t)i] - 2.0 * d[(size_t)i] - d[(size_t)i + 1]) / h[(size_t)i];
            c[3] = (d[(size_t)i] + d[(size_t)i + 1] - 2.0 * delta[(size_t)i]) / (h[(size_t)i] * h[(size_t)i]);
        }
        slope_left = d[0]; slope_right = d[(size_t)m - 1];
    }
    // the ends: the value at the end knot, and with linear extrapolation the slope of the adjacent segment there
    C[0] = V[0];
    if (extrapolation == FM_TABLE_LINEAR_EXTRAPOLATION) { C[1] = slope_left; C[m * 4 + 1] = slope_right; }
    if (derivative == 1)
        for (int s = 0; s <= m; ++s) { double* c = C + s * 4; c[0] = c[1]; c[1] = 2.0 * c[2]; c[2] = 3.0 * c[3]; c[3] = 0.0; }
}

// the definition over an array: out[f][p] for table f of coefficients[n_tables][m + 1][4]
inline void table_apply_host(const float* x, int64_t n, const double* knots, int m, const double* coefficients, int n_tables, float* const* out)
{
    tableCheckApply(knots, m, coefficients, n_tables, out);
    if (!x) throw std::invalid_argument("tabulated function: null pointer: x");
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("tabulated function: of " + std::to_string(n) + " elements (1 … 2^31)");
    for (int f = 0; f < n_tables; ++f) if (!out[f]) throw std::invalid_argument("tabulated function: null pointer: out[" + std::to_string(f) + "]");
    for (int64_t p = 0; p < n; ++p) {
        const double X = (double)x[p];
        const int s = X != X ? 0 : fm_table_segment_plain(knots, m, X);
        const double a = knots[s > 0 ? s - 1 : 0];
        for (int f = 0; f < n_tables; ++f) out[f][p] = fm_table_value(coefficients + ((size_t)f * (m + 1) + s) * 4, X, a);
    }
}

} // namespace fmhost
#endif
