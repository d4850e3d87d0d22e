// cross_order_kernel.hip — fm_cross_order_kernel<P, W, PAIRS> and fm_cross_select_kernel for gfx950 (MI355X, CDNA4): the K values of every
// path sorted by the 32-bit key of host/block_order.hpp with the slot as the tie-break, in a lane's registers, and of the sorted pairs the
// selected ranks as values and as slots; and the element of one of K vectors that a per-path index names.  DESIGN.md §4.24; contract:
// include/fmhip.h; definition: host/cross_order.hpp, whose network (fm_cross_network) is compiled here; launchers: cross_order_kernel.h;
// engine side: cross_order_engine.hpp.
//
// A lane owns W paths (cross_paths_per_lane): four with 16-byte loads and stores while its words fit in about 64 registers, two with
// 8-byte ones up to about 128, one above (32 pairs of one path are 64 registers).  A wave's K loads are K coalesced rows of 1 KiB, 512 B
// resp. 256 B.  A vector's storage is a multiple of 256 bytes (Pool::alloc rounds the capacity), so the last group is read and written
// whole: what lies past n is inside the buffer, and every bit pattern is a value the key takes.  The loop is grid-stride with a capped
// grid.  P is the power of two >= K.  ALL P loads of a group are issued before the first key is formed — none sits behind a branch on K,
// which would make every load wait for the one before it (the first build of this kernel did: one s_waitcnt vmcnt(0) per row): the
// addresses K … P−1 repeat address K−1 (a hit in the cache: fewer than K such loads), and what they bring is replaced by the pad — the
// NaN key with the word's own position as the slot: pads sort behind the real NaNs (whose slots are smaller), so positions < K hold the
// path's own pairs.  With no index wanted (PAIRS = false) the network runs on the keys alone: equal keys have equal bits.
// No LDS, no atomics, no workgroup waits for another, no scratch: every register array is indexed by unrolled, compile-time indices — the
// sorted position r is a compile-time constant, and WHICH outputs want it is a uniform loop over the launch's arguments (value_begin,
// index_begin: the selectors ordered by rank).  Only the selected ranks are stored.
// fm_cross_select_kernel: one path per lane; the index is range-checked (fm_cross_select_slot) BEFORE it picks one of the K base addresses
// among the launch's arguments; a lane whose index names no slot loads nothing and stores the quiet NaN.
// The kernels trust their arguments: the launchers refuse what cross_order_shape_ok / cross_select_shape_ok refuse.
#include <hip/hip_runtime.h>

#include "cross_order_kernel.h"

namespace fm {

typedef uint32_t co_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t co_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t __attribute__((address_space(1))) co_g1;              // global memory: global_load / global_store, not flat
typedef co_u32x2 __attribute__((address_space(1))) co_g2;
typedef co_u32x4 __attribute__((address_space(1))) co_g4;

template <int W> struct CoGroup;
template <> struct CoGroup<1> {
    uint32_t x[1];
    __device__ __forceinline__ void load(uint64_t base, int64_t g) { x[0] = reinterpret_cast<const co_g1*>(base)[g]; }
    __device__ __forceinline__ void store(uint64_t base, int64_t g) const { reinterpret_cast<co_g1*>(base)[g] = x[0]; }
};
template <> struct CoGroup<2> {
    uint32_t x[2];
    __device__ __forceinline__ void load(uint64_t base, int64_t g) { const co_u32x2 q = reinterpret_cast<const co_g2*>(base)[g]; x[0] = q[0]; x[1] = q[1]; }
    __device__ __forceinline__ void store(uint64_t base, int64_t g) const { co_u32x2 q; q[0] = x[0]; q[1] = x[1]; reinterpret_cast<co_g2*>(base)[g] = q; }
};
template <> struct CoGroup<4> {
    uint32_t x[4];
    __device__ __forceinline__ void load(uint64_t base, int64_t g) { const co_u32x4 q = reinterpret_cast<const co_g4*>(base)[g]; x[0] = q[0]; x[1] = q[1]; x[2] = q[2]; x[3] = q[3]; }
    __device__ __forceinline__ void store(uint64_t base, int64_t g) const { co_u32x4 q; q[0] = x[0]; q[1] = x[1]; q[2] = x[2]; q[3] = x[3]; reinterpret_cast<co_g4*>(base)[g] = q; }
};

template <bool PAIRS> struct CoWord;
template <> struct CoWord<false> { typedef uint32_t type; static __device__ __forceinline__ uint32_t make(uint32_t key, uint32_t) { return key; } };
template <> struct CoWord<true> { typedef uint64_t type; static __device__ __forceinline__ uint64_t make(uint32_t key, uint32_t slot) { return fmhost::fm_cross_pair(key, slot); } };

template <int P, int W, bool PAIRS>
__global__ void __launch_bounds__(FM_CROSS_BLOCK) fm_cross_order_kernel(const DevCrossOrderArgs A)
{
    typedef typename CoWord<PAIRS>::type word;
    const uint32_t K = A.n_vectors;
    const int64_t groups = (A.n + W - 1) / W, stride = (int64_t)gridDim.x * FM_CROSS_BLOCK;
#pragma unroll 1
    for (int64_t g = (int64_t)blockIdx.x * FM_CROSS_BLOCK + threadIdx.x; g < groups; g += stride) {
        CoGroup<W> in[P];
#pragma unroll
        for (int i = 0; i < P; ++i) in[i].load(A.v[i], g);                             // (v[K … P−1] = v[K−1]: no branch between the loads)
        word a[W][P];
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const bool real = (uint32_t)i < K;                                         // (K is the launch's: a scalar condition)
#pragma unroll
            for (int w = 0; w < W; ++w) a[w][i] = CoWord<PAIRS>::make(real ? fmhost::fm_order_key(in[i].x[w]) : fmhost::FM_ORDER_NAN_KEY, (uint32_t)i);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) fmhost::fm_cross_network<P>(a[w]);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            if ((uint32_t)r < K) {
                if (A.n_values) {
                    CoGroup<W> y;
#pragma unroll
                    for (int w = 0; w < W; ++w) y.x[w] = fmhost::fm_order_bits(fmhost::fm_cross_pair_key(a[w][r]));
#pragma unroll 1
                    for (uint32_t o = A.value_begin[r]; o < A.value_begin[r + 1]; ++o) y.store(A.value_out[o], g);
                }
                if (PAIRS) {
                    CoGroup<W> y;
#pragma unroll
                    for (int w = 0; w < W; ++w) y.x[w] = __float_as_uint((float)(uint32_t)a[w][r]);
#pragma unroll 1
                    for (uint32_t o = A.index_begin[r]; o < A.index_begin[r + 1]; ++o) y.store(A.index_out[o], g);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(FM_CROSS_BLOCK) fm_cross_select_kernel(const DevCrossSelectArgs A)
{
    const float* __restrict__ index = reinterpret_cast<const float*>(A.index);
    uint32_t* __restrict__ out = reinterpret_cast<uint32_t*>(A.out);
    const int K = (int)A.n_vectors;
    const int64_t stride = (int64_t)gridDim.x * FM_CROSS_BLOCK;
#pragma unroll 1
    for (int64_t p = (int64_t)blockIdx.x * FM_CROSS_BLOCK + threadIdx.x; p < A.n; p += stride) {
        const int j = fmhost::fm_cross_select_slot(index[p], K);
        uint32_t u = fmhost::FM_ORDER_NAN_BITS;
        if (j >= 0) u = reinterpret_cast<const uint32_t*>(A.v[j])[p];                  // 0 <= j < K: checked above
        out[p] = u;
    }
}

template <int P, bool PAIRS>
static void co_launch(const DevCrossOrderArgs& a, hipStream_t st)
{
    constexpr int W = cross_paths_per_lane(P, PAIRS);
    hipLaunchKernelGGL((fm_cross_order_kernel<P, W, PAIRS>), dim3(cross_blocks(a.n, W)), dim3(FM_CROSS_BLOCK), 0, st, a);
}
template <bool PAIRS>
static void co_launch_padded(const DevCrossOrderArgs& a, hipStream_t st)
{
    switch (fmhost::fm_cross_padded((int)a.n_vectors)) {
    case 2:  co_launch<2, PAIRS>(a, st); break;
    case 4:  co_launch<4, PAIRS>(a, st); break;
    case 8:  co_launch<8, PAIRS>(a, st); break;
    case 16: co_launch<16, PAIRS>(a, st); break;
    default: co_launch<32, PAIRS>(a, st); break;
    }
}

hipError_t launch_cross_order(const DevCrossOrderArgs& a, hipStream_t st)
{
    if (!cross_order_shape_ok(a)) return hipErrorInvalidValue;
    if (a.n_indices) co_launch_padded<true>(a, st); else co_launch_padded<false>(a, st);
    return hipGetLastError();
}

hipError_t launch_cross_select(const DevCrossSelectArgs& a, hipStream_t st)
{
    if (!cross_select_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fm_cross_select_kernel, dim3(cross_blocks(a.n, 1)), dim3(FM_CROSS_BLOCK), 0, st, a);
    return hipGetLastError();
}

} // namespace fm
