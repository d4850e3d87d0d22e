// sobol.hpp — the definition of the quasi-Monte-Carlo Brownian motion: Sobol' points (Joe & Kuo's direction numbers, Gray-code order), a
// digital shift, the inverse normal CDF and a Brownian-bridge (or increment-by-increment) construction.  DESIGN.md §4.12.  ONE header that
// the host (g++, hipcc -x c++) and the device (csrc/sobol_kernel.hip) both compile, as host/gamma_icdf.hpp is: what a draw goes through is
// written with integer operations, + − × / and sqrt only, every operation rounded once (builds: -ffp-contract=off, no fast-math), so the
// increments of the device EQUAL the host's, every one.
//
//   point           path p (global index) uses i = p + 1 (the origin is skipped); x(i, d) = XOR over the set bits j of i ^ (i >> 1) of v[d][j]
//   shift           randomize = 1: shift[d] = MT19937(seed).next32() >> 2, d = 0, 1, … in order; randomize = 0: all 0
//   uniform         u = (double)(x ^ shift[d]) · 2^-30 + 2^-31: exact, never 0 or 1
//   normal          z = fm_normal_quantile(u)
//   construction    FMHIP_SOBOL_INCREMENTAL (0): dimension step · n_factors + f, increment z · sqrt(dt[step])
//                   FMHIP_SOBOL_BRIDGE (1): node k of factor f uses dimension k · n_factors + f; node 0 is W(t_n) = sqrt(t_n − t_0) · z, the
//                   others fill midpoints breadth first: W_m = a·W_l + (1 − a)·W_r + sd·z.  a, 1 − a and sd are computed HERE, by the host,
//                   once per node, and only read by the device.  Increment of step j: W_(j+1) − W_j, narrowed to fp32 once.
// The device walks a PLAN (SobolPlan::ops) that this header builds: the same nodes in time order, every W in one of a few slots, so that a
// lane holds at most ⌈log2 n⌉ + 2 values; the host definition below walks the breadth-first node list and a whole W array instead.  Both
// evaluate fm_bridge_node on the same operands, so the order of the walk does not show in the bits (tests compare them).
#pragma once
#include "gamma_icdf.hpp"
#include "mersenne.hpp"
#include "sobol_directions.hpp"

#include <stdexcept>
#include <string>
#include <vector>

namespace fmhost {

constexpr int FM_SOBOL_INCREMENTAL = 0, FM_SOBOL_BRIDGE = 1;
constexpr int64_t FM_SOBOL_INDEX_LIMIT = int64_t(1) << FM_SOBOL_BITS;       // i = path + 1 < 2^30
constexpr int FM_SOBOL_MAX_SLOTS = 16;                                      // values a lane holds at once (n <= 1024 steps needs 12)

// ---------------------------------------------------------------- what the device compiles too

// x(i, d) from the 30 direction words of dimension d
FM_HD inline uint32_t fm_sobol_point(const uint32_t* v, uint32_t i)
{
    uint32_t g = i ^ (i >> 1), x = 0;
    for (int j = 0; g; ++j, g >>= 1) if (g & 1u) x ^= v[j];
    return x;
}

FM_HD inline double fm_sobol_uniform(uint32_t x) { return (double)x * 0x1.0p-30 + 0x1.0p-31; }

// a bridge node from the values at the ends of its interval
FM_HD inline double fm_bridge_node(double a, double b, double sd, double w_left, double w_right, double z)
{
    const double left = a * w_left, right = b * w_right, noise = sd * z;
    return (left + right) + noise;
}

// One step of the plan the device walks, per factor, in this order.  32 bytes, read by every lane alike.
enum { FM_SOBOL_OP_TERMINAL = 0,        // W[out] = sd · z(node)
       FM_SOBOL_OP_NODE = 1,            // W[out] = fm_bridge_node(a, b, sd, W[left], W[right], z(node))
       FM_SOBOL_OP_EMIT = 2,            // increment of step `node` = W[right] − W[left]
       FM_SOBOL_OP_DRAW = 3 };          // increment of step `node` = z(node) · sd                               (incremental construction)
struct SobolOp {
    uint8_t  kind, out, left, right;    // slots
    uint32_t node;                      // the bridge node or the time step; the dimension is node · n_factors + factor
    double   a, b, sd;
};

// ---------------------------------------------------------------- host only

// v[d][j], d < 1024, j < 30: the compact table expanded by the recurrence, once
inline const uint32_t* sobolDirections()
{
    static const std::vector<uint32_t> words = [] {
        std::vector<uint32_t> v((size_t)FM_SOBOL_DIMS * FM_SOBOL_BITS);
        for (int d = 0; d < FM_SOBOL_DIMS; ++d) {
            const uint16_t* row = FM_SOBOL_COMPACT + FM_SOBOL_ROW_START[d];
            const int s = row[0]; const uint32_t a = row[1];
            uint32_t* w = v.data() + (size_t)d * FM_SOBOL_BITS;
            if (s == 0) { for (int j = 0; j < FM_SOBOL_BITS; ++j) w[j] = 1u << (FM_SOBOL_BITS - 1 - j); continue; }
            for (int j = 0; j < s && j < FM_SOBOL_BITS; ++j) w[j] = (uint32_t)row[2 + j] << (FM_SOBOL_BITS - 1 - j);
            for (int j = s; j < FM_SOBOL_BITS; ++j) {
                uint32_t x = w[j - s] ^ (w[j - s] >> s);
                for (int k = 1; k < s; ++k) if ((a >> (s - 1 - k)) & 1u) x ^= w[j - k];
                w[j] = x;
            }
        }
        return v;
    }();
    return words.data();
}

inline std::vector<uint32_t> sobolShifts(int32_t seed, int randomize, int n_dims)
{
    std::vector<uint32_t> shift((size_t)n_dims, 0u);
    if (randomize) { MT19937 mt((int64_t)seed); for (int d = 0; d < n_dims; ++d) shift[(size_t)d] = mt.next32() >> 2; }
    return shift;
}

struct SobolNode { int left, mid, right; double a, b, sd; };      // breadth-first; node 0: the terminal value (left = 0, mid = right = n)

struct SobolPlan {
    int n_steps = 0, n_factors = 0, construction = 0, n_slots = 0;
    std::vector<double> times;          // t_0 = 0, t_(k+1) = t_k + dt[k]
    std::vector<SobolNode> nodes;       // bridge: n_steps nodes
    std::vector<SobolOp> ops;           // what the device walks
};

// The checks, for the host entry point and the engine alike; throws std::invalid_argument.  `dt` may be null only when it is not read.
inline void sobolCheck(int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt)
{
    if (n_steps <= 0 || n_factors <= 0 || n_paths < 0 || !dt) throw std::invalid_argument("bad description of the Sobol' Brownian motion");
    if (construction != FM_SOBOL_INCREMENTAL && construction != FM_SOBOL_BRIDGE) throw std::invalid_argument("unknown construction " + std::to_string(construction) + " (0: incremental, 1: Brownian bridge)");
    if (randomize != 0 && randomize != 1) throw std::invalid_argument("randomize is 0 or 1, not " + std::to_string(randomize));
    if ((int64_t)n_steps * n_factors > FM_SOBOL_DIMS) throw std::invalid_argument(std::to_string(n_steps) + " steps of " + std::to_string(n_factors) + " factors need " + std::to_string((int64_t)n_steps * n_factors) + " dimensions; the direction numbers reach " + std::to_string(FM_SOBOL_DIMS));
    if (path_offset < 0) throw std::invalid_argument("negative path offset");
    if (path_offset >= FM_SOBOL_INDEX_LIMIT || n_paths >= FM_SOBOL_INDEX_LIMIT - path_offset) throw std::invalid_argument("path offset + paths must stay below 2^30, the length of the sequence");
    for (int i = 0; i < n_steps; ++i) {
        const bool finite = dt[i] - dt[i] == 0.0;
        if (!finite || dt[i] < 0.0 || (construction == FM_SOBOL_BRIDGE && dt[i] == 0.0))
            throw std::invalid_argument("time step " + std::to_string(i) + " is not " + (construction == FM_SOBOL_BRIDGE ? "positive" : "non-negative") + " and finite");
    }
}

// Checked arguments -> the nodes and the device's plan
inline SobolPlan sobolPlan(int construction, int n_steps, int n_factors, const double* dt)
{
    SobolPlan P;
    P.n_steps = n_steps; P.n_factors = n_factors; P.construction = construction;
    P.times.assign((size_t)n_steps + 1, 0.0);
    for (int k = 0; k < n_steps; ++k) P.times[(size_t)k + 1] = P.times[(size_t)k] + dt[k];
    if (construction == FM_SOBOL_INCREMENTAL) {
        for (int k = 0; k < n_steps; ++k) {
            SobolOp o{}; o.kind = FM_SOBOL_OP_DRAW; o.node = (uint32_t)k; o.sd = std::sqrt(dt[k]);
            P.ops.push_back(o);
        }
        return P;
    }
    const std::vector<double>& t = P.times;
    const int n = n_steps;
    std::vector<int> node_of((size_t)n + 1, -1);                // time index -> the node that draws it
    P.nodes.push_back({ 0, n, n, 0.0, 0.0, std::sqrt(t[(size_t)n] - t[0]) });
    node_of[(size_t)n] = 0;
    std::vector<std::pair<int, int>> queue{ { 0, n } };
    for (size_t head = 0; head < queue.size(); ++head) {
        const int l = queue[head].first, r = queue[head].second;
        if (r - l < 2) continue;
        const int m = (l + r) / 2;
        const double span = t[(size_t)r] - t[(size_t)l], up = t[(size_t)r] - t[(size_t)m], down = t[(size_t)m] - t[(size_t)l];
        const double a = up / span;
        node_of[(size_t)m] = (int)P.nodes.size();
        P.nodes.push_back({ l, m, r, a, 1.0 - a, std::sqrt(down * up / span) });
        queue.push_back({ l, m }); queue.push_back({ m, r });
    }
    // the same nodes in time order: slot 0 holds W_0 = 0 throughout, slot 1 W_n; a midpoint takes a free slot and gives it back when the
    // interval to its right is done
    std::vector<int> free_slots;
    for (int s = FM_SOBOL_MAX_SLOTS - 1; s >= 2; --s) free_slots.push_back(s);
    int high = 2;
    { SobolOp o{}; o.kind = FM_SOBOL_OP_TERMINAL; o.out = 1; o.node = 0; o.sd = P.nodes[0].sd; P.ops.push_back(o); }
    struct Frame { int l, r, slot_l, slot_r, stage, slot_m; };
    std::vector<Frame> stack{ { 0, n, 0, 1, 0, -1 } };
    while (!stack.empty()) {
        Frame& f = stack.back();
        if (f.r - f.l == 1) {
            SobolOp o{}; o.kind = FM_SOBOL_OP_EMIT; o.left = (uint8_t)f.slot_l; o.right = (uint8_t)f.slot_r; o.node = (uint32_t)f.l;
            P.ops.push_back(o); stack.pop_back(); continue;
        }
        const int m = (f.l + f.r) / 2;
        if (f.stage == 0) {
            if (free_slots.empty()) throw std::invalid_argument("the Brownian bridge needs more than " + std::to_string(FM_SOBOL_MAX_SLOTS) + " values per path at once");
            f.slot_m = free_slots.back(); free_slots.pop_back();
            if (f.slot_m + 1 > high) high = f.slot_m + 1;
            const SobolNode& N = P.nodes[(size_t)node_of[(size_t)m]];
            SobolOp o{}; o.kind = FM_SOBOL_OP_NODE; o.out = (uint8_t)f.slot_m; o.left = (uint8_t)f.slot_l; o.right = (uint8_t)f.slot_r;
            o.node = (uint32_t)node_of[(size_t)m]; o.a = N.a; o.b = N.b; o.sd = N.sd;
            P.ops.push_back(o);
            f.stage = 1;
            const Frame child{ f.l, m, f.slot_l, f.slot_m, 0, -1 };
            stack.push_back(child);
        } else if (f.stage == 1) {
            f.stage = 2;
            const Frame child{ m, f.r, f.slot_m, f.slot_r, 0, -1 };
            stack.push_back(child);
        } else {
            free_slots.push_back(f.slot_m);
            stack.pop_back();
        }
    }
    P.n_slots = high;
    return P;
}

// What the kernel relies on in a plan and does not check itself: slots below n_slots, steps and dimensions in range, every step emitted once
inline bool sobolPlanOk(const SobolOp* ops, size_t n_ops, int n_steps, int n_factors, int n_slots)
{
    if (n_slots < 0 || n_slots > FM_SOBOL_MAX_SLOTS || n_steps <= 0 || n_factors <= 0 || (int64_t)n_steps * n_factors > FM_SOBOL_DIMS) return false;
    std::vector<char> emitted((size_t)n_steps, 0);
    for (size_t k = 0; k < n_ops; ++k) {
        const SobolOp& o = ops[k];
        if (o.kind > FM_SOBOL_OP_DRAW || o.node >= (uint32_t)n_steps) return false;
        if (o.kind != FM_SOBOL_OP_DRAW && (o.out >= n_slots || o.left >= n_slots || o.right >= n_slots)) return false;
        if ((o.kind == FM_SOBOL_OP_TERMINAL || o.kind == FM_SOBOL_OP_NODE) && o.out == 0) return false;       // slot 0 stays W_0 = 0
        if (o.kind == FM_SOBOL_OP_EMIT || o.kind == FM_SOBOL_OP_DRAW) { if (emitted[o.node]) return false; emitted[o.node] = 1; }
    }
    for (char e : emitted) if (!e) return false;
    return true;
}

// u_out[k · n_dims + d] = the uniform of point first_index + k (index i: 1 is the first point after the origin) in dimension d
inline void sobolPoints(int n_dims, int64_t first_index, int64_t count, int32_t seed, int randomize, double* u_out)
{
    if (n_dims <= 0 || n_dims > FM_SOBOL_DIMS) throw std::invalid_argument(std::to_string(n_dims) + " dimensions: the direction numbers reach 1 … " + std::to_string(FM_SOBOL_DIMS));
    if (randomize != 0 && randomize != 1) throw std::invalid_argument("randomize is 0 or 1, not " + std::to_string(randomize));
    if (count < 0 || first_index < 0 || first_index >= FM_SOBOL_INDEX_LIMIT || count > FM_SOBOL_INDEX_LIMIT - first_index || (count > 0 && !u_out))
        throw std::invalid_argument("the points of a Sobol' sequence have indices 0 … 2^30 − 1");
    const uint32_t* v = sobolDirections();
    const std::vector<uint32_t> shift = sobolShifts(seed, randomize, n_dims);
    for (int64_t k = 0; k < count; ++k)
        for (int d = 0; d < n_dims; ++d)
            u_out[(size_t)k * n_dims + d] = fm_sobol_uniform(fm_sobol_point(v + (size_t)d * FM_SOBOL_BITS, (uint32_t)(first_index + k)) ^ shift[(size_t)d]);
}

// out[(step · n_factors + factor) · n_paths + k] = the increment of path path_offset + k, a double (the device narrows it to fp32).
inline void sobolIncrements(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, double* out)
{
    sobolCheck(randomize, construction, n_steps, n_factors, n_paths, path_offset, dt);
    if (n_paths > 0 && !out) throw std::invalid_argument("bad description of the Sobol' Brownian motion");
    const SobolPlan P = sobolPlan(construction, n_steps, n_factors, dt);
    const uint32_t* v = sobolDirections();
    const std::vector<uint32_t> shift = sobolShifts(seed, randomize, n_steps * n_factors);
    auto z = [&](uint32_t i, int d) { return fm_normal_quantile(fm_sobol_uniform(fm_sobol_point(v + (size_t)d * FM_SOBOL_BITS, i) ^ shift[(size_t)d])); };
    std::vector<double> W((size_t)n_steps + 1);
    for (int64_t k = 0; k < n_paths; ++k) {
        const uint32_t i = (uint32_t)(path_offset + k + 1);
        for (int f = 0; f < n_factors; ++f) {
            if (construction == FM_SOBOL_INCREMENTAL) {
                for (int step = 0; step < n_steps; ++step)
                    out[((size_t)step * n_factors + f) * (size_t)n_paths + (size_t)k] = z(i, step * n_factors + f) * P.ops[(size_t)step].sd;
                continue;
            }
            W[0] = 0.0;
            W[(size_t)n_steps] = P.nodes[0].sd * z(i, f);
            for (size_t node = 1; node < P.nodes.size(); ++node) {
                const SobolNode& N = P.nodes[node];
                W[(size_t)N.mid] = fm_bridge_node(N.a, N.b, N.sd, W[(size_t)N.left], W[(size_t)N.right], z(i, (int)node * n_factors + f));
            }
            for (int step = 0; step < n_steps; ++step)
                out[((size_t)step * n_factors + f) * (size_t)n_paths + (size_t)k] = W[(size_t)step + 1] - W[(size_t)step];
        }
    }
}

} // namespace fmhost
