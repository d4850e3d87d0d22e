// sort_kernel.hip — a stable least-significant-digit radix sort of (key, path index) pairs for gfx950 (MI355X, CDNA4), and the kernels that
// turn its permutation into results.  DESIGN.md §4.16; contract: include/fmhip.h; launchers and chunk arithmetic: sort_kernel.h; engine
// side: sort_engine.hpp.
//
// Key: os_key of §4.7 (os_device.hpp) — unsigned order of the keys = order of java.util.Arrays.sort(float[]), every NaN the last key.
// Four passes of 8-bit digits, each three kernels chained on the stream:
//   count    workgroup w counts the digits of ITS chunk — sort_chunk_tiles(n) consecutive tiles of the current order — in LDS (integer adds
//            with the wave-level peeling of §4.7) and stores its row table[w][0..255] with plain stores.  No global atomic.
//   offsets  one workgroup turns the table into first destinations: an exclusive scan in (digit, workgroup) order.
//   scatter  workgroup w walks its chunk tile by tile, in order.  Inside a tile wave v owns the elements [512·v, 512·v + 512) and takes them in
//            eight rounds of 64 consecutive elements; the rank of an element among the EQUAL digits before it in the tile is
//            (equal digits in earlier waves) + (in earlier rounds of its wave) + (in lower lanes of its round), the last from eight ballots.
//            The tile is put in digit order in LDS, then written: consecutive lanes write consecutive addresses of one digit's run.
// Equal digits keep their incoming order at every level — lane, round, wave, tile, workgroup — so the sort is stable: equal keys end in
// ascending path order, NaNs (one key) among them.
//
// No workgroup waits for another inside a kernel: there is no flag, no arrival counter and no look-back anywhere in this file; the order
// count → offsets → scatter → next pass is the stream's.  Integers only, no atomics on global memory at all.  Positions are uint32
// (n <= 2^31 - 1, checked by the launchers and before them by the engine); lanes past n are masked, and every store is bounded by n.
#include <hip/hip_runtime.h>

#include "sort_kernel.h"
#include "os_device.hpp"

namespace fm {

typedef uint32_t st_u32x4 __attribute__((ext_vector_type(4)));
typedef float st_f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t ST_WAVES = FM_SORT_BLOCK / 64;
constexpr uint32_t ST_WAVE_ELEMS = FM_SORT_TILE / ST_WAVES;        // 512 consecutive elements of a tile per wave
static_assert(FM_SORT_BINS == FM_SORT_BLOCK, "thread d of a workgroup owns digit d");
static_assert(ST_WAVE_ELEMS == 64 * FM_SORT_ITEMS, "a wave takes its elements in FM_SORT_ITEMS rounds of 64");

// Exclusive prefix of v over the threads 0 … 255 of the workgroup (every thread of the workgroup calls; threads above 255 pass 0 and get
// nothing of use).  wave_total: four words of LDS, free to be written again after the caller's next barrier.
__device__ __forceinline__ uint32_t st_scan256(const uint32_t v, uint32_t* wave_total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= (uint32_t)off) incl += up;
    }
    if (lane == 63u && wave < ST_WAVES) wave_total[wave] = incl;
    __syncthreads();
    uint32_t before = 0u;
#pragma unroll
    for (uint32_t w = 0; w < ST_WAVES; ++w) if (w < wave) before += wave_total[w];
    return before + incl - v;
}

__global__ void __launch_bounds__(FM_SORT_BLOCK) fm_sort_count_kernel(const DevSortPassArgs A)
{
    __shared__ uint32_t h[FM_SORT_BINS];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t n = A.n, shift = A.shift;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_SORT_TILE - 1) / FM_SORT_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const st_u32x4* __restrict__ p = reinterpret_cast<const st_u32x4*>(A.src_key);      // 16-byte loads: storage is 256-byte aligned and padded
    const bool from_floats = A.from_floats != 0u;
    for (uint32_t tile = t0; tile < t1; ++tile) {
        st_u32x4 v[2]; uint32_t e0[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            e0[u] = tile * (uint32_t)FM_SORT_TILE + ((uint32_t)u * FM_SORT_BLOCK + threadIdx.x) * 4u;      // < n + tile < 2^32
            v[u] = p[e0[u] < n ? e0[u] / 4u : 0u];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = from_floats ? os_key(__uint_as_float(v[u][j])) : v[u][j];
                os_lds_add(h, (key >> shift) & 255u, e0[u] + (uint32_t)j < n);
            }
        }
    }
    __syncthreads();
    A.table[(size_t)blockIdx.x * FM_SORT_BINS + threadIdx.x] = h[threadIdx.x];
}

// table[w][d]: count → the first destination of workgroup w's elements of digit d = Σ counts of (d', w') before (d, w) in (digit, workgroup)
// order.  ONE workgroup of 1024 lanes: lane (q, d) owns digit d in the q-th quarter of the workgroups; consecutive lanes read consecutive words.
constexpr int ST_OFFSETS_BLOCK = 1024;
__global__ void __launch_bounds__(ST_OFFSETS_BLOCK) fm_sort_offsets_kernel(uint32_t* __restrict__ table, const uint32_t blocks)
{
    __shared__ uint32_t part[4][FM_SORT_BINS];
    __shared__ uint32_t wave_total[ST_WAVES];
    const uint32_t d = threadIdx.x & 255u, q = threadIdx.x >> 8;
    const uint32_t w0 = (uint32_t)(((uint64_t)blocks * q) / 4u), w1 = (uint32_t)(((uint64_t)blocks * (q + 1u)) / 4u);
    uint32_t sum = 0u;
#pragma unroll 8
    for (uint32_t w = w0; w < w1; ++w) sum += table[(size_t)w * FM_SORT_BINS + d];
    part[q][d] = sum;
    __syncthreads();
    uint32_t total = 0u;
    if (q == 0u) total = ((part[0][d] + part[1][d]) + part[2][d]) + part[3][d];
    const uint32_t first = st_scan256(total, wave_total);
    if (q == 0u) {
        uint32_t run = first;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const uint32_t c = part[k][d]; part[k][d] = run; run += c; }
    }
    __syncthreads();
    uint32_t run = part[q][d];
#pragma unroll 8
    for (uint32_t w = w0; w < w1; ++w) {
        const uint32_t c = table[(size_t)w * FM_SORT_BINS + d];
        table[(size_t)w * FM_SORT_BINS + d] = run;
        run += c;
    }
}

__global__ void __launch_bounds__(FM_SORT_BLOCK) fm_sort_scatter_kernel(const DevSortPassArgs A)
{
    __shared__ uint32_t wave_hist[ST_WAVES][FM_SORT_BINS];      // per wave: digits seen so far in the tile; then the wave's first position per digit
    __shared__ uint32_t glob[FM_SORT_BINS];                     // destination of position p of the ordered tile, digit d: glob[d] + p
    __shared__ uint32_t key_s[FM_SORT_TILE], idx_s[FM_SORT_TILE];
    __shared__ uint32_t wave_total[ST_WAVES];
    const uint32_t n = A.n, shift = A.shift;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lower = (1ull << lane) - 1ull;
    const uint32_t tiles = (uint32_t)(((uint64_t)n + FM_SORT_TILE - 1) / FM_SORT_TILE);
    const uint32_t t0 = blockIdx.x * A.chunk_tiles, t1 = t0 + A.chunk_tiles < tiles ? t0 + A.chunk_tiles : tiles;
    const bool from_floats = A.from_floats != 0u, write_keys = A.write_keys != 0u;
    const uint32_t* __restrict__ src_key = reinterpret_cast<const uint32_t*>(A.src_key);
    const uint32_t* __restrict__ src_idx = reinterpret_cast<const uint32_t*>(A.src_idx);
    uint32_t* __restrict__ dst_key = reinterpret_cast<uint32_t*>(A.dst_key);
    uint32_t* __restrict__ dst_idx = reinterpret_cast<uint32_t*>(A.dst_idx);
    uint32_t* const my_hist = wave_hist[wave];
    uint32_t run = A.table[(size_t)blockIdx.x * FM_SORT_BINS + threadIdx.x];      // thread d: where this workgroup's next element of digit d goes
#pragma unroll 1
    for (uint32_t tile = t0; tile < t1; ++tile) {
        const uint32_t base = tile * (uint32_t)FM_SORT_TILE;                      // < n
        const uint32_t in_tile = n - base < (uint32_t)FM_SORT_TILE ? n - base : (uint32_t)FM_SORT_TILE;
        // the wave's 512 consecutive elements, round j = 64 consecutive ones: 4-byte loads, because the element order IS the lane order
        uint32_t key[FM_SORT_ITEMS], idx[FM_SORT_ITEMS], rank[FM_SORT_ITEMS];
#pragma unroll
        for (int j = 0; j < FM_SORT_ITEMS; ++j) {
            const uint32_t e = base + wave * ST_WAVE_ELEMS + (uint32_t)j * 64u + lane;
            const bool valid = e < n;
            const uint32_t raw = src_key[valid ? e : 0u];
            key[j] = from_floats ? os_key(__uint_as_float(raw)) : raw;
            idx[j] = from_floats ? e : src_idx[valid ? e : 0u];
        }
#pragma unroll
        for (int k = 0; k < FM_SORT_BINS / 64; ++k) my_hist[(uint32_t)k * 64u + lane] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < FM_SORT_ITEMS; ++j) {
            const bool valid = base + wave * ST_WAVE_ELEMS + (uint32_t)j * 64u + lane < n;
            const uint32_t d = (key[j] >> shift) & 255u;
            uint64_t same = __ballot(valid);                     // the lanes of the round that hold the same digit: eight ballots
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t with = __ballot(bit);
                same &= bit ? with : ~with;
            }
            const uint32_t earlier = (uint32_t)__popcll(same & lower);
            const uint32_t seen = my_hist[d];                    // equal digits in the wave's earlier rounds (every lane of `same` reads the same word)
            rank[j] = seen + earlier;
            __builtin_amdgcn_wave_barrier();
            if (valid && earlier == 0u) my_hist[d] = seen + (uint32_t)__popcll(same);      // the first lane of each digit
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        // thread d: the tile's elements of digit d per wave → the first position of each wave's run in the ordered tile, and where the run goes
        {
            const uint32_t d = threadIdx.x;
            uint32_t c[ST_WAVES], total = 0u;
#pragma unroll
            for (uint32_t w = 0; w < ST_WAVES; ++w) { c[w] = wave_hist[w][d]; total += c[w]; }
            const uint32_t first = st_scan256(total, wave_total);
            uint32_t at = first;
#pragma unroll
            for (uint32_t w = 0; w < ST_WAVES; ++w) { wave_hist[w][d] = at; at += c[w]; }
            glob[d] = run - first;
            run += total;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FM_SORT_ITEMS; ++j) {
            const bool valid = base + wave * ST_WAVE_ELEMS + (uint32_t)j * 64u + lane < n;
            if (valid) {
                const uint32_t at = my_hist[(key[j] >> shift) & 255u] + rank[j];
                if (at < (uint32_t)FM_SORT_TILE) { key_s[at] = key[j]; idx_s[at] = idx[j]; }
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FM_SORT_ITEMS; ++j) {
            const uint32_t p = (uint32_t)j * FM_SORT_BLOCK + threadIdx.x;
            if (p < in_tile) {
                const uint32_t k = key_s[p];
                const uint32_t to = glob[(k >> shift) & 255u] + p;
                if (to < n) {
                    if (write_keys) dst_key[to] = k;
                    dst_idx[to] = idx_s[p];
                }
            }
        }
        // (the next tile writes wave_hist rows of its own wave only before the next barrier, and key_s, idx_s, glob and wave_total behind it)
    }
}

// out[k][r] = src[k][perm[r]]: four consecutive r per lane — one 16-byte load of the permutation, one 16-byte store per vector
__global__ void __launch_bounds__(256) fm_sort_gather_kernel(const DevSortGatherArgs A)
{
    const uint32_t n = A.n;
    const uint64_t quads = ((uint64_t)n + 3u) / 4u;
    const st_u32x4* __restrict__ perm = reinterpret_cast<const st_u32x4*>(A.perm);
    for (uint64_t i4 = (uint64_t)blockIdx.x * 256u + threadIdx.x; i4 < quads; i4 += (uint64_t)gridDim.x * 256u) {
        st_u32x4 p = perm[i4];
#pragma unroll
        for (int j = 0; j < 4; ++j) if (i4 * 4u + (uint32_t)j >= n || p[j] >= n) p[j] = 0u;      // tail lanes, and no load ever leaves the vector
        for (uint32_t k = 0; k < A.count; ++k) {
            const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(A.src[k]);
            st_u32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[p[j]];
            reinterpret_cast<st_u32x4*>(A.dst[k])[i4] = v;       // (storage is padded to 256 bytes: the last quad is inside it)
        }
    }
}

__global__ void __launch_bounds__(256) fm_sort_scores_kernel(const uint32_t* __restrict__ perm, float* __restrict__ out, const uint32_t n)
{
    const uint64_t quads = ((uint64_t)n + 3u) / 4u;
    const double dn = (double)n;
    for (uint64_t i4 = (uint64_t)blockIdx.x * 256u + threadIdx.x; i4 < quads; i4 += (uint64_t)gridDim.x * 256u) {
        const st_u32x4 p = reinterpret_cast<const st_u32x4*>(perm)[i4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t r = i4 * 4u + (uint32_t)j;
            if (r < n && p[j] < n) out[p[j]] = (float)(((double)r + 0.5) / dn);
        }
    }
}

__global__ void __launch_bounds__(256) fm_sort_read_elements_kernel(const float* __restrict__ v, const uint32_t* __restrict__ pos, const uint32_t count, double* __restrict__ out_host)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < count) out_host[j] = (double)v[pos[j]];
    __threadfence_system();
}

__global__ void __launch_bounds__(64) fm_sort_done_kernel(uint64_t* done_flag, const uint64_t done_value)
{
    if (threadIdx.x == 0u) __hip_atomic_store(done_flag, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

static uint32_t st_stream_blocks(uint64_t quads)
{
    const uint64_t b = (quads + 255u) / 256u;
    return (uint32_t)(b < 1u ? 1u : b > (uint64_t)FM_SORT_STREAM_MAX_BLOCKS ? (uint64_t)FM_SORT_STREAM_MAX_BLOCKS : b);
}

hipError_t launch_sort_pass(const DevSortPassArgs& a, hipStream_t st)
{
    if (!sort_pass_shape_ok(a)) return hipErrorInvalidValue;
    const uint32_t blocks = sort_blocks((int64_t)a.n);
    hipLaunchKernelGGL(fm_sort_count_kernel, dim3(blocks), dim3(FM_SORT_BLOCK), 0, st, a);
    hipLaunchKernelGGL(fm_sort_offsets_kernel, dim3(1), dim3(ST_OFFSETS_BLOCK), 0, st, a.table, blocks);
    hipLaunchKernelGGL(fm_sort_scatter_kernel, dim3(blocks), dim3(FM_SORT_BLOCK), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sort_gather(const DevSortGatherArgs& a, hipStream_t st)
{
    if (a.n == 0u || a.n > (uint32_t)FM_SORT_MAX_N || a.count == 0u || a.count > 1u + (uint32_t)FM_SORT_MAX_VALUES || !a.perm) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < a.count; ++k) if (!a.src[k] || !a.dst[k] || a.src[k] == a.dst[k]) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_sort_gather_kernel, dim3(st_stream_blocks(((uint64_t)a.n + 3u) / 4u)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sort_scores(uint64_t perm, uint64_t out, uint32_t n, hipStream_t st)
{
    if (n == 0u || n > (uint32_t)FM_SORT_MAX_N || !perm || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_sort_scores_kernel, dim3(st_stream_blocks(((uint64_t)n + 3u) / 4u)), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(perm), reinterpret_cast<float*>(out), n);
    return hipGetLastError();
}

hipError_t launch_sort_read_elements(uint64_t v, const uint32_t* pos, uint32_t count, double* out_host, hipStream_t st)
{
    if (!v || !pos || count == 0u || !out_host) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_sort_read_elements_kernel, dim3((count + 255u) / 256u), dim3(256), 0, st, reinterpret_cast<const float*>(v), pos, count, out_host);
    return hipGetLastError();
}

hipError_t launch_sort_done(uint64_t* done_flag, uint64_t done_value, hipStream_t st)
{
    if (!done_flag) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_sort_done_kernel, dim3(1), dim3(64), 0, st, done_flag, done_value);
    return hipGetLastError();
}

} // namespace fm
