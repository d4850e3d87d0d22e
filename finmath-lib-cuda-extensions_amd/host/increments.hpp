// increments.hpp — header-only definition of independent increments with a law per (time step, factor), drawn from finmath-lib's
// MT19937 stream through an inverse cumulative distribution function: the general case of which the Brownian motion of mersenne.hpp is
// one.  Shared by libfmhip (csrc/abi.cpp → fmhip_increments_host; csrc/mt_generate_engine.hpp → the device pass, which must
// reproduce these numbers), by the null-device stand-in of the kernel and by the C++ host mirror (host/independent_increments.hpp).
//
// It stands in for finmath-lib's IndependentIncrementsFromICDF (one MersenneTwister.nextDouble() per increment, pushed through an
// inverse CDF chosen per time step and factor) and for JumpProcessIncrements / the three-factor layout of MonteCarloMertonModel on top
// of it (factor 0 a Brownian increment, factor 1 a standard normal jump size, factor 2 a Poisson jump count with mean λ·dt)
// [unverified: finmath-lib is not vendored; class names, the draw order and the layout are restated from its documentation, as
// everything in mersenne.hpp is].
//
// One draw per increment, path-major (for path, for step, for factor), u = MT19937::nextDouble() in [0, 1), u = 0 possible.
//   NORMAL   inverseNormalCdf(u) · a                a >= 0: sqrt(dt) for a Brownian factor, 1 for a jump size
//   UNIFORM  a + (b − a) · u                        a <= b, finite; every operation rounded once, in this order
//   POISSON  min { k >= 0 : F[k] >= u }             a = the mean λ·dt, 0 <= a <= 128; F a table built here, once per distinct mean
//   GAMMA    fm_inverse_gamma_cdf(a, consts, u) · b a = the shape, 0.01 <= a <= 1000, b = the scale, finite and positive (kind 4)
//   EXPONENTIAL  −fm_log64(1 − u) / a               a = the rate, finite and positive (kind 5; kind 3 is no law)
// The last two are defined in gamma_icdf.hpp, a header the device compiles too, without a library transcendental: equal by construction.
// `consts` is what depends on the shape alone (lgamma(shape), 1/shape, …), computed here once per distinct shape; it lies in `tables`
// beside the Poisson tables, addressed the same way.
// The Poisson table is plain fp64: p = F[0] = exp(−a); p = p·a/k, F[k] = F[k−1] + p; it ends at the first k past the mode with
// F[k] == F[k−1] or F[k] >= 1 − 2^-53, and its last entry is replaced by 1.0, so every u < 1 finds a k.  Whoever draws — this header or
// the device — only compares u with these doubles: the counts are equal by construction.  The cap keeps a table under 300 entries.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "gamma_icdf.hpp"
#include "mersenne.hpp"

namespace fmhost {

constexpr int32_t LAW_NORMAL = 0, LAW_UNIFORM = 1, LAW_POISSON = 2, LAW_GAMMA = 4, LAW_EXPONENTIAL = 5;
constexpr double POISSON_MEAN_CAP = 128.0;
constexpr int64_t INCREMENT_STREAMS_CAP = int64_t(1) << 24;           // laws (steps · factors) per call
constexpr int64_t INCREMENT_WORDS_CAP = int64_t(1) << 44;             // the jump-ahead table reaches 2^44 words of the stream
constexpr size_t INCREMENT_TABLE_DOUBLES_CAP = size_t(1) << 16;       // all distinct Poisson tables and gamma constants of a call together

inline std::vector<double> poissonTable(double mean) {
    std::vector<double> F;
    double p = std::exp(-mean);
    F.push_back(p);
    if (mean > 0.0)
        for (int k = 1;; ++k) {
            p = p * mean / k;
            F.push_back(F.back() + p);
            if ((double)k > mean && (F[(size_t)k] == F[(size_t)k - 1] || F[(size_t)k] >= 1.0 - 0x1.0p-53)) break;
        }
    F.back() = 1.0;
    return F;
}

// min { k : F[k] >= u } for u < 1 = F[len − 1]
inline int poissonFromTable(const double* F, int len, double u) {
    int lo = 0, hi = len - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (F[mid] < u) lo = mid + 1; else hi = mid; }
    return lo;
}

// What fm_inverse_gamma_cdf reads per shape (gamma_icdf.hpp: FM_GC_…).  lgamma_r: std::lgamma writes the global signgam.
inline std::vector<double> gammaConsts(double shape) {
    std::vector<double> c((size_t)FM_GAMMA_CONSTS);
    int sign = 0;
    c[FM_GC_LGAMMA] = ::lgamma_r(shape, &sign);
    c[FM_GC_INV_SHAPE] = 1.0 / shape;
    c[FM_GC_LGAMMA1] = ::lgamma_r(shape + 1.0, &sign);
    c[FM_GC_WH_CENTRE] = 1.0 - 1.0 / (9.0 * shape);
    c[FM_GC_WH_SLOPE] = 1.0 / (3.0 * std::sqrt(shape));
    c[FM_GC_SPLIT] = shape <= 1.0 ? 1.0 - shape * (0.253 + shape * 0.12) : 1.0;
    return c;
}

// The laws of a call, checked, with the Poisson tables built and shared between equal means.
struct IncrementLaws {
    struct Law { int32_t kind; uint32_t table_len; uint32_t table_offset; uint32_t reserved; double a, b; };   // the device's descriptor too
    std::vector<Law> laws;              // [n_steps · n_factors], index step · n_factors + factor
    std::vector<double> tables;         // every distinct table, one behind the other
    double draw(size_t stream, double u) const {
        const Law& L = laws[stream];
        if (L.kind == LAW_NORMAL) return inverseNormalCdf(u) * L.a;
        if (L.kind == LAW_UNIFORM) { const double width = L.b - L.a; const double scaled = width * u; return L.a + scaled; }
        if (L.kind == LAW_GAMMA) return fm_inverse_gamma_cdf(L.a, tables.data() + L.table_offset, u) * L.b;
        if (L.kind == LAW_EXPONENTIAL) return fm_exponential_icdf(L.a, u);
        return (double)poissonFromTable(tables.data() + L.table_offset, (int)L.table_len, u);
    }
};
static_assert(sizeof(IncrementLaws::Law) == 32, "the descriptor is 32 bytes on the host and on the device");

// Everything that can be said about a call without a device, in ONE place for the host entry point and the engine: throws
// std::invalid_argument, otherwise returns the laws.  Paths path_offset … path_offset + n_paths are asked for.
inline IncrementLaws checkedIncrementLaws(int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const int32_t* kinds, const double* a, const double* b) {
    if (n_steps <= 0 || n_factors <= 0 || n_paths < 0 || path_offset < 0 || n_paths > (int64_t(1) << 31) || !kinds || !a || !b)
        throw std::invalid_argument("bad description of the increments");
    const int64_t n_streams = (int64_t)n_steps * n_factors;
    if (n_streams > INCREMENT_STREAMS_CAP) throw std::invalid_argument("more than 2^24 increments per path");
    const int64_t limit = INCREMENT_WORDS_CAP / (2 * n_streams);
    if (path_offset > limit || n_paths > limit - path_offset)
        throw std::invalid_argument("the Mersenne-Twister stream is entered by jump-ahead, which reaches 2^44 words: path offset + paths <= " + std::to_string(limit) + " at this shape");
    IncrementLaws out;
    out.laws.resize((size_t)n_streams);
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> seen;             // bits of a mean → (offset, length) of its table
    std::map<uint64_t, std::pair<uint32_t, uint32_t>> seen_shapes;      // bits of a shape → (offset, length) of its constants
    for (size_t s = 0; s < (size_t)n_streams; ++s) {
        IncrementLaws::Law& L = out.laws[s];
        L.kind = kinds[s]; L.a = a[s]; L.b = b[s]; L.table_len = 0; L.table_offset = 0; L.reserved = 0;
        const std::string where = " (step " + std::to_string(s / (size_t)n_factors) + ", factor " + std::to_string(s % (size_t)n_factors) + ")";
        if (L.kind == LAW_NORMAL) {
            if (!(L.a >= 0.0)) throw std::invalid_argument("normal law: the scale is negative or not a number" + where);
            L.b = 0.0;
        } else if (L.kind == LAW_UNIFORM) {
            if (!std::isfinite(L.a) || !std::isfinite(L.b)) throw std::invalid_argument("uniform law: the bounds are not finite" + where);
            if (L.a > L.b) throw std::invalid_argument("uniform law: lower bound above upper bound" + where);
        } else if (L.kind == LAW_POISSON) {
            if (!(L.a >= 0.0)) throw std::invalid_argument("Poisson law: the mean is negative or not a number" + where);
            if (L.a > POISSON_MEAN_CAP) throw std::invalid_argument("Poisson law: the mean is above 128" + where);
            if (L.a == 0.0) L.a = 0.0;                                  // −0 and +0 share a table
            L.b = 0.0;
            uint64_t bits; std::memcpy(&bits, &L.a, 8);
            auto it = seen.find(bits);
            if (it == seen.end()) {
                const std::vector<double> F = poissonTable(L.a);
                if (out.tables.size() + F.size() > INCREMENT_TABLE_DOUBLES_CAP)
                    throw std::invalid_argument("the distinct Poisson means of this call need more than 2^16 table entries");
                it = seen.emplace(bits, std::make_pair((uint32_t)out.tables.size(), (uint32_t)F.size())).first;
                out.tables.insert(out.tables.end(), F.begin(), F.end());
            }
            L.table_offset = it->second.first; L.table_len = it->second.second;
        } else if (L.kind == LAW_GAMMA) {
            if (!std::isfinite(L.a) || !(L.a > 0.0)) throw std::invalid_argument("gamma law: the shape is not a positive finite number" + where);
            if (L.a < FM_GAMMA_SHAPE_MIN || L.a > FM_GAMMA_SHAPE_MAX) throw std::invalid_argument("gamma law: the shape is outside 0.01 … 1000" + where);
            if (!std::isfinite(L.b) || !(L.b > 0.0)) throw std::invalid_argument("gamma law: the scale is not a positive finite number" + where);
            uint64_t bits; std::memcpy(&bits, &L.a, 8);
            auto it = seen_shapes.find(bits);
            if (it == seen_shapes.end()) {
                const std::vector<double> c = gammaConsts(L.a);
                if (out.tables.size() + c.size() > INCREMENT_TABLE_DOUBLES_CAP)
                    throw std::invalid_argument("the Poisson tables and gamma constants of this call need more than 2^16 table entries" + where);
                it = seen_shapes.emplace(bits, std::make_pair((uint32_t)out.tables.size(), (uint32_t)c.size())).first;
                out.tables.insert(out.tables.end(), c.begin(), c.end());
            }
            L.table_offset = it->second.first; L.table_len = it->second.second;
        } else if (L.kind == LAW_EXPONENTIAL) {
            if (!std::isfinite(L.a) || !(L.a > 0.0)) throw std::invalid_argument("exponential law: the rate is not a positive finite number" + where);
            L.b = 0.0;
        } else throw std::invalid_argument("unknown law " + std::to_string(L.kind) + where);
    }
    return out;
}

// out[(step*n_factors + factor)*n_paths + path], doubles (host).  No device involved.  The definition.
inline void independentIncrements(int32_t seed, int n_steps, int n_factors, int64_t n_paths, const int32_t* kinds, const double* a, const double* b, double* out) {
    const IncrementLaws laws = checkedIncrementLaws(n_steps, n_factors, n_paths, 0, kinds, a, b);
    if (!out && n_paths > 0) throw std::invalid_argument("bad description of the increments");
    MT19937 mt((int64_t)seed);                                  // the int seed of the finmath constructor, widened
    const size_t n_streams = laws.laws.size();
    for (int64_t path = 0; path < n_paths; ++path)
        for (size_t s = 0; s < n_streams; ++s)
            out[s * (size_t)n_paths + (size_t)path] = laws.draw(s, mt.nextDouble());
}

} // namespace fmhost
