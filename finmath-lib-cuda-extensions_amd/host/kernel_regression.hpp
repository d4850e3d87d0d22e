// kernel_regression.hpp — kernel regression in one dimension: the DEFINITION of the local moments of up to four vectors at a grid of points
// of a key vector (include/fmhip.h: fmhip_kernel_moments, fmhip_kernel_moments_host), in ONE header that the host (g++,
// hipcc -x c++) and the device (csrc/kreg_kernel.hip) both compile, the ONE argument check the host and the device entry points use, and
// the local constant / local linear fit made of the sums.  No device, no library: plain C++.
//
// Points p_q (Q of them, 1 … 256, finite, non-decreasing) and bandwidths h_q (finite, > 0).  Per point, one fp64 rounding each:
//   lower_q = p_q − h_q,  upper_q = p_q + h_q,  rh_q = 1.0 / h_q;  lower and upper must both be non-decreasing in q.
// Membership is defined by these two arrays and nothing else: with xd = (double)key[i], element i is a member of point q iff
//   lower_q < xd && xd < upper_q.  A NaN or infinite key is a member of no point.  Both arrays are monotone, so the members of xd are exactly
//   q ∈ [a, b),  a = #{ q : upper_q <= xd },  b = #{ q : lower_q < xd }   (fm_kernel_range; the device finds the two by branch-free searches).
// Weight of a member, in fp64, every operation rounded on its own (builds: -ffp-contract=off, no fast-math):
//   d = xd − p_q;  u = d·rh_q;  t = 1 − u·u;  w = 1 | 1 − |u| | t | t·t | (t·t)·t;  w = w < 0 ? 0 : w.
// Terms of a member, yd_m = (double)y_m[i]:   order 0: [w, w·yd_0, …]            (1 + n_y entries per point)
//                                              order 1: [w, e1 = w·d, e1·d, w·yd_0, …, e1·yd_0, …]   (3 + 2·n_y entries)
// The result is the fp64 SUMS over the members; the normalisation (3/4, 1/(n·h)) is the caller's.  Only + − × |·|, comparisons and integer
// operations, and one division per point on the host: the device's terms EQUAL the host's, the sums differ by the order of the additions.
// A Gaussian kernel is not offered: its support is not compact, so every (element, point) pair would contribute.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define FM_KREG_HD __host__ __device__
#else
#define FM_KREG_HD
#endif

namespace fmhost {

constexpr int FM_KERNEL_MAX_POINTS = 256;
constexpr int FM_KERNEL_MAX_Y = 4;
constexpr int FM_KERNEL_MAX_ENTRIES_PER_POINT = 3 + 2 * FM_KERNEL_MAX_Y;

enum { FM_KERNEL_UNIFORM = 0, FM_KERNEL_TRIANGULAR = 1, FM_KERNEL_EPANECHNIKOV = 2, FM_KERNEL_QUARTIC = 3, FM_KERNEL_TRIWEIGHT = 4 };      // = FMHIP_KERNEL_*

FM_KREG_HD inline int fm_kernel_entries(int order, int n_y) { return order == 0 ? 1 + n_y : 3 + 2 * n_y; }

// the weight of a member at distance d of a point with reciprocal bandwidth rh
FM_KREG_HD inline double fm_kernel_weight(int kernel, double d, double rh)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double u = d * rh;
    const double uu = u * u;
    const double t = 1.0 - uu;
    double w;
    if (kernel == FM_KERNEL_UNIFORM) w = 1.0;
    else if (kernel == FM_KERNEL_TRIANGULAR) w = 1.0 - (u < 0.0 ? -u : u);
    else if (kernel == FM_KERNEL_EPANECHNIKOV) w = t;
    else if (kernel == FM_KERNEL_QUARTIC) w = t * t;
    else { const double tt = t * t; w = tt * t; }
    return w < 0.0 ? 0.0 : w;                       // a boundary member can round to a hair below zero
}

// terms[fm_kernel_entries(order, n_y)] of one member: w its weight, d = xd − p_q, yd[n_y]
FM_KREG_HD inline void fm_kernel_terms(int order, int n_y, double w, double d, const double* yd, double* terms)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    terms[0] = w;
    if (order == 0) {
        for (int m = 0; m < n_y; ++m) terms[1 + m] = w * yd[m];
        return;
    }
    const double e1 = w * d;
    terms[1] = e1;
    terms[2] = e1 * d;
    for (int m = 0; m < n_y; ++m) { terms[3 + m] = w * yd[m]; terms[3 + n_y + m] = e1 * yd[m]; }
}

// [a, b): the points xd is a member of.  NaN: every comparison is false, a = b = 0; −inf: 0, 0; +inf: Q, Q.
FM_KREG_HD inline void fm_kernel_range(const double* lower, const double* upper, int Q, double xd, int* a_out, int* b_out)
{
    int lo = 0, hi = Q;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (upper[mid] <= xd) lo = mid + 1; else hi = mid; }
    *a_out = lo;
    lo = 0; hi = Q;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (lower[mid] < xd) lo = mid + 1; else hi = mid; }
    *b_out = lo;
}

} // namespace fmhost

#if !defined(__HIP_DEVICE_COMPILE__)
#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

inline bool kernel_finite(double d) { return d - d == 0.0; }

// lower, upper, rh [Q] from the points and the bandwidths: one rounding each
inline void kernel_edges(const double* points, const double* bandwidths, int Q, double* lower, double* upper, double* rh)
{
    for (int q = 0; q < Q; ++q) { lower[q] = points[q] - bandwidths[q]; upper[q] = points[q] + bandwidths[q]; rh[q] = 1.0 / bandwidths[q]; }
}

// What can be said about a call without looking at a vector.  T: a handle or a pointer (0 / nullptr is no vector).
template <class T>
inline void kernelMomentsCheck(T key, const double* points, const double* bandwidths, int n_points, int kernel, int order, const T* y, int n_y, const void* sums_out)
{
    if (n_points < 1 || n_points > FM_KERNEL_MAX_POINTS) throw std::invalid_argument("kernel moments at " + std::to_string(n_points) + " points: 1 … " + std::to_string(FM_KERNEL_MAX_POINTS));
    if (n_y < 0 || n_y > FM_KERNEL_MAX_Y) throw std::invalid_argument("kernel moments of " + std::to_string(n_y) + " vectors: 0 … " + std::to_string(FM_KERNEL_MAX_Y));
    if (order != 0 && order != 1) throw std::invalid_argument("kernel moments of order " + std::to_string(order) + ": 0 (local constant) or 1 (local linear)");
    if (kernel < FM_KERNEL_UNIFORM || kernel > FM_KERNEL_TRIWEIGHT) throw std::invalid_argument("kernel moments: kernel " + std::to_string(kernel) + " (FMHIP_KERNEL_UNIFORM … FMHIP_KERNEL_TRIWEIGHT)");
    if (!points || !bandwidths || (n_y > 0 && !y) || !sums_out) throw std::invalid_argument("kernel moments: a required pointer is NULL");
    if (!key) throw std::invalid_argument("kernel moments: the key is a vector");
    for (int m = 0; m < n_y; ++m) if (!y[m]) throw std::invalid_argument("kernel moments: y[" + std::to_string(m) + "] is no vector");
    double lower_before = 0.0, upper_before = 0.0;
    for (int q = 0; q < n_points; ++q) {
        if (!kernel_finite(points[q])) throw std::invalid_argument("kernel moments: point " + std::to_string(q) + " is not finite");
        if (!kernel_finite(bandwidths[q]) || !(bandwidths[q] > 0.0)) throw std::invalid_argument("kernel moments: bandwidth " + std::to_string(q) + " is not a finite number above 0");
        if (q > 0 && points[q] < points[q - 1]) throw std::invalid_argument("kernel moments: the points are not sorted at " + std::to_string(q));
        const double lower = points[q] - bandwidths[q], upper = points[q] + bandwidths[q], rh = 1.0 / bandwidths[q];
        if (!kernel_finite(lower) || !kernel_finite(upper) || !kernel_finite(rh)) throw std::invalid_argument("kernel moments: the support of point " + std::to_string(q) + " is not finite");
        if (q > 0 && (lower < lower_before || upper < upper_before))
            throw std::invalid_argument("kernel moments: the supports' ends are not non-decreasing at point " + std::to_string(q) + " (the bandwidths change too fast)");
        lower_before = lower; upper_before = upper;
    }
}

// The definition: sums_out[n_points][fm_kernel_entries(order, n_y)]; a point's members are added in path order.
inline void kernel_moments_host(const float* key, int64_t n, const double* points, const double* bandwidths, int n_points, int kernel, int order,
                                const float* const* y, int n_y, double* sums_out)
{
    kernelMomentsCheck<const float*>(key, points, bandwidths, n_points, kernel, order, y, n_y, sums_out);
    if (n < 1 || n > (int64_t(1) << 31)) throw std::invalid_argument("kernel moments of " + std::to_string(n) + " elements (1 … 2^31)");
    const int Q = n_points, qe = fm_kernel_entries(order, n_y);
    std::vector<double> lower((size_t)Q), upper((size_t)Q), rh((size_t)Q);
    kernel_edges(points, bandwidths, Q, lower.data(), upper.data(), rh.data());
    for (size_t i = 0; i < (size_t)Q * qe; ++i) sums_out[i] = 0.0;
    double yd[FM_KERNEL_MAX_Y] = {}, terms[FM_KERNEL_MAX_ENTRIES_PER_POINT];
    for (int64_t p = 0; p < n; ++p) {
        const double xd = (double)key[p];
        int a, b;
        fm_kernel_range(lower.data(), upper.data(), Q, xd, &a, &b);
        if (a >= b) continue;
        for (int m = 0; m < n_y; ++m) yd[m] = (double)y[m][p];
        for (int q = a; q < b; ++q) {
            const double d = xd - points[q];
            fm_kernel_terms(order, n_y, fm_kernel_weight(kernel, d, rh[(size_t)q]), d, yd, terms);
            double* s = sums_out + (size_t)q * qe;
            for (int e = 0; e < qe; ++e) s[e] = s[e] + terms[e];
        }
    }
}

// The fit at the points, from the sums.  values_out[n_y][Q]; slopes_out[n_y][Q] or nullptr (order 0: zeros).
//   order 0: Wy / W.   order 1: the 2×2 solve of [[W, Wd], [Wd, Wdd]] — value = (Wdd·Wy − Wd·Wdy) / det, slope = (W·Wdy − Wd·Wy) / det,
//   det = W·Wdd − Wd·Wd — and order 0 (slope 0) where det is not above 1e-12·W·Wdd.
// A point with W == 0 (or a W that is no positive finite number) has no fit: it is filled by linear interpolation in p between its nearest
// fitted neighbours, or by the value of the nearest one beyond the outermost fitted points (and where the two neighbours share their p, the
// left one's value).  No fitted point at all: std::invalid_argument.
inline void kernel_local_fit(const double* sums, int order, int n_y, const double* points, int n_points, double* values_out, double* slopes_out)
{
    if (!sums || !points || !values_out) throw std::invalid_argument("kernel fit: a required pointer is NULL");
    if (n_points < 1 || n_points > FM_KERNEL_MAX_POINTS || n_y < 1 || n_y > FM_KERNEL_MAX_Y || (order != 0 && order != 1)) throw std::invalid_argument("kernel fit: counts out of range");
    const int Q = n_points, qe = fm_kernel_entries(order, n_y);
    std::vector<char> fitted((size_t)Q, 0);
    bool any = false;
    for (int q = 0; q < Q; ++q) {
        const double* s = sums + (size_t)q * qe;
        const double W = s[0];
        fitted[(size_t)q] = (W > 0.0 && kernel_finite(W)) ? 1 : 0;
        any = any || fitted[(size_t)q];
        for (int m = 0; m < n_y; ++m) {
            double value = 0.0, slope = 0.0;
            if (fitted[(size_t)q]) {
                if (order == 0) value = s[1 + m] / W;
                else {
                    const double Wd = s[1], Wdd = s[2], Wy = s[3 + m], Wdy = s[3 + n_y + m];
                    const double det = W * Wdd - Wd * Wd;
                    if (det > 1e-12 * W * Wdd) { value = (Wdd * Wy - Wd * Wdy) / det; slope = (W * Wdy - Wd * Wy) / det; }
                    else value = Wy / W;
                }
            }
            values_out[(size_t)m * Q + q] = value;
            if (slopes_out) slopes_out[(size_t)m * Q + q] = slope;
        }
    }
    if (!any) throw std::invalid_argument("kernel fit: no point has a member with a positive weight");
    for (int q = 0; q < Q; ++q) {
        if (fitted[(size_t)q]) continue;
        int l = q - 1, r = q + 1;
        while (l >= 0 && !fitted[(size_t)l]) --l;
        while (r < Q && !fitted[(size_t)r]) ++r;
        for (int m = 0; m < n_y; ++m) {
            double* v = values_out + (size_t)m * Q;
            double* sl = slopes_out ? slopes_out + (size_t)m * Q : nullptr;
            if (l >= 0 && r < Q && points[r] > points[l]) {
                const double f = (points[q] - points[l]) / (points[r] - points[l]);
                v[q] = v[l] + f * (v[r] - v[l]);
                if (sl) sl[q] = sl[l] + f * (sl[r] - sl[l]);
            }
            else { const int from = l >= 0 ? l : r; v[q] = v[from]; if (sl) sl[q] = sl[from]; }
        }
    }
}

} // namespace fmhost
#endif
