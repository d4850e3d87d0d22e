// mt_bm_kernel.hip — finmath-lib's Mersenne-Twister Brownian increments generated on the device (gfx950), to the bits of the host
// generator (host/mersenne.hpp: MT19937 → nextDouble → AS 241 → · sqrt(dt) → fp32).  DESIGN.md §4.9.
//
// The output stream (two 32-bit words per draw, path-major: path, step, factor) is cut into segments of L = 2^j words.  Workgroup k owns
// the paths whose first word lies in [k·L, (k+1)·L) — words counted from the first word of local path 0, to which the engine has already
// moved the seeded state (fm_mt_jump_kernel) — and
//   prologue: jumps from there to k·L by the set bits of k: for each, 19936 raw words behind the state through a window in LDS and 624
//             XOR sums over the set bits of g_(j+b)(t) = t^(2^(j+b)) mod φ(t) (fm_mt_jump_table.hpp; read wave-uniformly), the three
//             accumulators of a lane in registers;
//   body:     512 new words per iteration in three dependent phases (x[m] needs x[m − 227]) into a ring in LDS, one draw per lane:
//             temper, 52-bit uniform, AS 241 in fp64 with separately rounded operations (the build's -ffp-contract=off), IEEE division and
//             square root, · sqrt(dt[step]) in fp64, ONE rounding to fp32 — the roundings of the host path plus its upload;
//   stores:   the stream is path-major, the vectors are [step·n_factors + factor][path]: a tile of paths is staged in LDS (two tiles, so
//             that an iteration may straddle a tile edge) and leaves as 16-byte nontemporal stores, runs of consecutive paths per vector;
//             a shape whose four paths do not fit a tile stores element by element.
// A workgroup discards the words before its first path and runs on past its segment's end to finish its last path.
//
// Contract (tests/test_gpu_mersenne_device.py): the uniforms are the host's bit for bit; a central draw (|u − 0.5| <= 0.425) goes through
// + − × / only and equals (float) of the host's double exactly; a tail draw goes through log, where the device library and the host's
// libm may differ by an fp64 ulp, which survives the rounding to fp32 with a probability of order 2^-29: equal, except that one in
// some 10^8 may differ by one fp32 ulp.
//
// fm_mt_icdf_kernel is the same pass with another last step: a law per stream — normal, uniform or Poisson — from a
// descriptor array (host/increments.hpp).  Poisson and uniform draws equal the host's exactly (a Poisson draw only compares the uniform
// with the host's fp64 table); normal draws are under the contract above.  Tests: tests/test_gpu_increments.py.
//
// fm_mt_levy_kernel is the pass once more, with the gamma and the exponential law beside those three.  Their definition
// (host/gamma_icdf.hpp) is compiled here and on the host from one text, with + − × /, sqrt and integer operations only: these draws are
// EQUAL to the host's.  An instantiation of its own, because the gamma branch is an fp64 iteration that costs registers: a call without
// these laws runs fm_mt_icdf_kernel as before.  Tests: tests/test_gpu_levy_increments.py.
#include <hip/hip_runtime.h>
#include "../host/gamma_icdf.hpp"
#define FM_MT_JUMP_TABLE_QUALIFIER __device__
#include "fm_mt_jump_table.hpp"
#include "mt_bm_kernel.h"

namespace fm {

typedef float mt_f32x4 __attribute__((ext_vector_type(4)));

constexpr int MT_BLOCK = FM_MT_BLOCK;
constexpr int MT_N = FM_MT_STATE_WORDS, MT_LAG = 227;                 // x[m] = x[m − 227] ^ twist(x[m − 624], x[m − 623])
constexpr int MT_DEGREE = 19937;
constexpr int MT_RING = 2048;                                         // body: words of the ring (624 of history + 512 new fit twice)
constexpr int MT_LDS_WORDS = MT_RING + 2 * FM_MT_TILE_FLOATS;         // 8448 words = 33 KB: four workgroups per CU
constexpr int MT_WINDOW_BLOCKS = 12;                                  // prologue: coefficients per pass = 12 x 624, window = 13 x 624 words
constexpr int MT_WINDOW = (MT_WINDOW_BLOCKS + 1) * MT_N;
static_assert(MT_WINDOW <= MT_LDS_WORDS && MT_WINDOW_BLOCKS * MT_N + 3 * MT_BLOCK <= MT_LDS_WORDS, "the window fits, and the third accumulator's loads of lanes >= 112 stay inside the array");
static_assert((MT_WINDOW_BLOCKS * MT_N) % 32 == 0, "a pass ends on a word of coefficients");

__device__ __forceinline__ uint32_t mt_twist(uint32_t hi, uint32_t lo, uint32_t far)
{
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// words [gen, gen + cnt) of a linear window, cnt <= 227 (they depend on nothing younger than gen − 227); ends in a barrier
__device__ __forceinline__ void mt_phase_linear(uint32_t* x, int gen, int cnt)
{
    const int t = (int)threadIdx.x;
    if (t < cnt) { const int m = gen + t; x[m] = mt_twist(x[m - MT_N], x[m - MT_N + 1], x[m - MT_LAG]); }
    __syncthreads();
}

// x[0 … 624) (LDS) ← the state 2^row words on.  Every lane keeps outputs k = t, t + 256, t + 512 (the last for t < 112).
__device__ void mt_jump_pow2(uint32_t* x, int row)
{
    const int t = (int)threadIdx.x;
    uint32_t acc0 = 0, acc1 = 0, acc2 = 0;
    const uint32_t* g = FM_MT_JUMP_TABLE[row];
    for (int base = 0; base < MT_DEGREE; base += MT_WINDOW_BLOCKS * MT_N) {
        // the window holds x[base … base + MT_WINDOW): 624 words are there, the rest follows in phases of 208 (= 624 / 3)
        for (int gen = MT_N; gen < MT_WINDOW; gen += 208) mt_phase_linear(x, gen, 208);
        const int w0 = base / 32;
        int w1 = w0 + MT_WINDOW_BLOCKS * MT_N / 32;
        if (w1 > FM_MT_JUMP_WORDS) w1 = FM_MT_JUMP_WORDS;
        const uint32_t* xt = x + t;
        for (int w = w0; w < w1; ++w, xt += 32) {
            const uint32_t bits = __builtin_amdgcn_readfirstlane(g[w]);
#pragma unroll
            for (int b = 0; b < 32; ++b)
                if (bits & (1u << b)) { acc0 ^= xt[b]; acc1 ^= xt[b + MT_BLOCK]; acc2 ^= xt[b + 2 * MT_BLOCK]; }
        }
        __syncthreads();
        // the last 624 words of the window open the next one
        uint32_t keep[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) { const int k = t + r * MT_BLOCK; keep[r] = k < MT_N ? x[MT_WINDOW_BLOCKS * MT_N + k] : 0u; }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; ++r) { const int k = t + r * MT_BLOCK; if (k < MT_N) x[k] = keep[r]; }
        __syncthreads();
    }
    x[t] = acc0; x[t + MT_BLOCK] = acc1;
    if (t + 2 * MT_BLOCK < MT_N) x[t + 2 * MT_BLOCK] = acc2;
    __syncthreads();
}

// x[0 … 624) ← the state `distance` words on, distance = steps · 2^row0
__device__ void mt_jump(uint32_t* x, uint64_t steps, int row0)
{
    for (int row = row0; steps != 0 && row < FM_MT_JUMP_COUNT; ++row, steps >>= 1)
        if (steps & 1u) mt_jump_pow2(x, row);
}

__device__ __forceinline__ void mt_load_state(uint32_t* x, const uint32_t* __restrict__ state)
{
    for (int k = (int)threadIdx.x; k < MT_N; k += MT_BLOCK) x[k] = state[k];
    __syncthreads();
}

__global__ void __launch_bounds__(MT_BLOCK) fm_mt_jump_kernel(const uint32_t* __restrict__ in, const uint64_t distance, uint32_t* __restrict__ out)
{
    __shared__ uint32_t x[MT_LDS_WORDS];
    mt_load_state(x, in);
    mt_jump(x, distance, 0);
    for (int k = (int)threadIdx.x; k < MT_N; k += MT_BLOCK) out[k] = x[k];
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= (y >> 11); y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= (y >> 18);
    return y;
}

// Wichura (1988), Algorithm AS 241, PPND16 — the operations of host/mersenne.hpp: inverseNormalCdf in their order, each rounded once
__device__ __forceinline__ double mt_inverse_normal(double p)
{
    if (!(p > 0.0)) return -__builtin_huge_val();                   // p = 0 (p < 1 always: 52 bits)
    const double q = p - 0.5;
    if (__builtin_fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r
                        + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r + 1.3314166789178437745e+2) * r + 3.3871328727963666080e0)
                 / (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r
                        + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r + 4.2313330701600911252e+1) * r + 1.0);
    }
    double r = sqrt(-log(q < 0 ? p : 1.0 - p));
    double val;
    if (r <= 5.0) {
        r -= 1.6;
        val = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r + 1.27045825245236838258e0) * r
                   + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r + 4.63033784615654529590e0) * r + 1.42343711074968357734e0)
            / (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r
                   + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r + 2.05319162663775882187e0) * r + 1.0);
    } else {
        r -= 5.0;
        val = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r
                   + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r + 5.46378491116411436990e0) * r + 6.65790464350110377720e0)
            / (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r
                   + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r + 5.99832206555887937690e-1) * r + 1.0);
    }
    return q < 0.0 ? -val : val;
}

// One staged tile leaves: tile[(path − tile_path)·S + s] → vector s, element path; paths outside [p_first, p_end) belong to a neighbour.
__device__ __forceinline__ void mt_flush_tile(const DevMtBmArgs& A, const float* tile, int64_t tile_path, int64_t p_first, int64_t p_end)
{
    const uint32_t S = A.n_streams, quads = A.tile_paths >> 2;
    const uint32_t total = S * quads;
    for (uint32_t idx = threadIdx.x; idx < total; idx += MT_BLOCK) {
        const uint32_t s = idx / quads, q = idx - s * quads;
        const int64_t p = tile_path + 4 * q;
        if (p + 4 <= p_first || p >= p_end) continue;
        const float* src = tile + (size_t)(4 * q) * S + s;
        const float v0 = src[0], v1 = src[S], v2 = src[2 * (size_t)S], v3 = src[3 * (size_t)S];
        float* dst = A.slab + (size_t)s * A.stride_floats + p;
        if (p >= p_first && p + 4 <= p_end) {
            __builtin_nontemporal_store(mt_f32x4{ v0, v1, v2, v3 }, reinterpret_cast<mt_f32x4*>(dst));
        } else {
            if (p >= p_first && p < p_end) __builtin_nontemporal_store(v0, dst);
            if (p + 1 >= p_first && p + 1 < p_end) __builtin_nontemporal_store(v1, dst + 1);
            if (p + 2 >= p_first && p + 2 < p_end) __builtin_nontemporal_store(v2, dst + 2);
            if (p + 3 >= p_first && p + 3 < p_end) __builtin_nontemporal_store(v3, dst + 3);
        }
    }
}

// The last step of a draw, u → the increment narrowed to fp32, for stream s.  Brownian: AS 241 times sqrt(dt[step]).
struct MtBrownianDraw {
    const double* sqrt_dt;
    __device__ __forceinline__ float operator()(double u, uint32_t s) const { return (float)(mt_inverse_normal(u) * sqrt_dt[s]); }
};

// A law per stream (host/increments.hpp: IncrementLaws::draw, operation for operation).  Lane t serves stream (e0 + t) mod S, so the
// law differs from lane to lane.  A Poisson draw only compares u with the doubles of the host's table, which lie in global memory: a
// call's tables are a few hundred bytes to 512 KB (more than LDS holds), every wave reads the same few lines, and they stay in the
// vector cache; a short table is walked from 0 (most of the mass of a small mean sits in the first entries), a long one bisected.
struct MtIcdfDraw {
    const DevMtLaw* laws;
    const double* tables;
    uint32_t linear_max;
    __device__ __forceinline__ float operator()(double u, uint32_t s) const
    {
        const DevMtLaw* L = laws + s;
        const int32_t kind = L->kind;
        if (kind == 0) return (float)(mt_inverse_normal(u) * L->a);
        if (kind == 1) { const double a = L->a; const double width = L->b - a; const double scaled = width * u; return (float)(a + scaled); }
        const uint32_t len = L->table_len;
        const double* F = tables + L->table_offset;
        uint32_t lo = 0;
        if (len <= linear_max) {
            while (lo + 1 < len && F[lo] < u) ++lo;                   // F[len − 1] = 1 > u is never read
        } else {
            uint32_t hi = len - 1;                                    // F[hi] >= u throughout
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (F[mid] < u) lo = mid + 1; else hi = mid; }
        }
        return (float)lo;
    }
};

// MtIcdfDraw's three laws and the two of host/gamma_icdf.hpp.  In a variance-gamma layout (gamma, normal, gamma, …) half the lanes of a
// wave iterate while the other half wait: the stream order is the contract, draws are not regrouped.
struct MtLevyDraw {
    MtIcdfDraw old;
    __device__ __forceinline__ float operator()(double u, uint32_t s) const
    {
        const DevMtLaw* L = old.laws + s;
        const int32_t kind = L->kind;
        if (kind == 4) return (float)(fmhost::fm_inverse_gamma_cdf(L->a, old.tables + L->table_offset, u) * L->b);
        if (kind == 5) return (float)fmhost::fm_exponential_icdf(L->a, u);
        return old(u, s);
    }
};

// The generation pass of one workgroup (header comment), shared by both kernels; `draw` is the last step.
template <class Draw>
__device__ __forceinline__ void mt_generate(const DevMtBmArgs& A, uint32_t* x, const Draw& draw)
{
    const uint32_t t = threadIdx.x;
    const uint64_t k = blockIdx.x;
    const uint32_t S = A.n_streams;
    const uint64_t words_per_path = 2ull * S;
    const uint64_t seg0 = k << A.segment_log2, seg1 = (k + 1) << A.segment_log2;
    // the paths whose first word lies in [seg0, seg1)
    const int64_t p_first = (int64_t)((seg0 + words_per_path - 1) / words_per_path);
    int64_t p_end = (int64_t)((seg1 + words_per_path - 1) / words_per_path);
    if (p_end > A.n_paths) p_end = A.n_paths;
    if (p_first >= p_end) return;                                   // workgroup-uniform, before any barrier

    mt_load_state(x, A.state);
    mt_jump(x, k, (int)A.segment_log2);

    // ---- body.  Ring position of a word = (624 + its number counted from seg0) mod 2048, in wrapping 32-bit arithmetic.
    uint32_t gen = MT_N;                                            // words generated so far (ring position of the next one)
    uint32_t cons = MT_N + (uint32_t)(p_first * words_per_path - seg0);  // ring position of the first word of this iteration's first draw: the words in front of the first path are generated and dropped
    const int64_t e_first = p_first * (int64_t)S, e_end = p_end * (int64_t)S;   // draws, counted from local path 0
    const uint32_t TP = A.tile_paths, TPS = TP * S;
    float* tiles = reinterpret_cast<float*>(x + MT_RING);
    // this lane's draw: stream s of path p; in tile mode its offset in the tile and the tile's parity
    uint32_t s = t % S;
    int64_t p = p_first + t / S;
    const uint32_t ds = MT_BLOCK % S, dp = MT_BLOCK / S;
    int64_t tile_path = 0, tile_e0 = 0;                             // the oldest tile not yet stored: its first path and first draw
    uint32_t off = 0, par = 0, flush_par = 0;
    if (TP) {
        tile_path = p_first - p_first % TP;
        tile_e0 = tile_path * (int64_t)S;
        off = (uint32_t)(e_first - tile_e0) + t;
        if (off >= TPS) { off -= TPS; par = 1; }
    }
    for (int64_t e0 = e_first; e0 < e_end; e0 += MT_BLOCK) {
        // words up to the end of this iteration's draws
        const uint32_t need = cons + 2 * MT_BLOCK;
        while ((int32_t)(need - gen) > 0) {
            uint32_t cnt = need - gen;
            if (cnt > 192u) cnt = 192u;
            if (t < cnt) { const uint32_t m = gen + t; x[m & (MT_RING - 1)] = mt_twist(x[(m - MT_N) & (MT_RING - 1)], x[(m - MT_N + 1) & (MT_RING - 1)], x[(m - MT_LAG) & (MT_RING - 1)]); }
            gen += cnt;
            __syncthreads();
        }
        if (e0 + t < e_end) {
            const uint2 w = *reinterpret_cast<const uint2*>(&x[(cons + 2 * t) & (MT_RING - 1)]);
            const uint64_t bits = ((uint64_t)(mt_temper(w.x) >> 6) << 26) | (uint64_t)(mt_temper(w.y) >> 6);
            const double u = (double)bits * 0x1.0p-52;
            const float z = draw(u, s);
            if (TP) tiles[par * FM_MT_TILE_FLOATS + off] = z;
            else __builtin_nontemporal_store(z, A.slab + (size_t)s * A.stride_floats + p);
        }
        cons = need;
        s += ds; p += dp;
        if (s >= S) { s -= S; ++p; }
        if (TP) {
            off += MT_BLOCK;
            if (off >= TPS) { off -= TPS; par ^= 1u; }
            // tiles this iteration completed (at most one, and at the end whatever is left) leave; the barriers of the next iteration's
            // phases stand between these reads and the next writes into the same tile
            const int64_t done = e0 + MT_BLOCK;
            while (tile_e0 < e_end && (tile_e0 + TPS <= done || done >= e_end) && tile_e0 < done) {
                __syncthreads();
                mt_flush_tile(A, tiles + flush_par * FM_MT_TILE_FLOATS, tile_path, p_first, p_end);
                tile_path += TP; tile_e0 += TPS; flush_par ^= 1u;
            }
        }
    }
}

__global__ void __launch_bounds__(MT_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) fm_mt_bm_kernel(const DevMtBmArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t x[MT_LDS_WORDS];
    mt_generate(A, x, MtBrownianDraw{ A.sqrt_dt });
}

__global__ void __launch_bounds__(MT_BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) fm_mt_icdf_kernel(const DevMtIcdfArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t x[MT_LDS_WORDS];
    mt_generate(A.g, x, MtIcdfDraw{ A.laws, A.tables, A.linear_max });
}

__global__ void __launch_bounds__(MT_BLOCK) fm_mt_levy_kernel(const DevMtIcdfArgs A)
{
    __shared__ __attribute__((aligned(16))) uint32_t x[MT_LDS_WORDS];
    mt_generate(A.g, x, MtLevyDraw{ { A.laws, A.tables, A.linear_max } });
}

hipError_t launch_mt_jump(const uint32_t* in, uint64_t distance, uint32_t* out, hipStream_t st)
{
    hipLaunchKernelGGL(fm_mt_jump_kernel, dim3(1), dim3(MT_BLOCK), 0, st, in, distance, out);
    return hipGetLastError();
}

hipError_t launch_mt_bm(const DevMtBmArgs& a, hipStream_t st)
{
    if (a.n_paths <= 0 || a.n_segments == 0) return hipSuccess;
    if (!mt_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_mt_bm_kernel, dim3(a.n_segments), dim3(MT_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mt_icdf(const DevMtIcdfArgs& a, hipStream_t st)
{
    if (a.g.n_paths <= 0 || a.g.n_segments == 0) return hipSuccess;
    if (!mt_shape_ok(a.g, &a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_mt_icdf_kernel, dim3(a.g.n_segments), dim3(MT_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_mt_levy(const DevMtIcdfArgs& a, hipStream_t st)
{
    if (a.g.n_paths <= 0 || a.g.n_segments == 0) return hipSuccess;
    if (!mt_shape_ok(a.g, &a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_mt_levy_kernel, dim3(a.g.n_segments), dim3(MT_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
