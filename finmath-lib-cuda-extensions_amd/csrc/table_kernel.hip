// table_kernel.hip — fm_table_apply_kernel for gfx950 (MI355X, CDNA4): up to four tabulated functions on the same knots applied to every
// element of a vector.  DESIGN.md §4.18; contract: include/fmhip.h; definition: host/tabulated_function.hpp (the segment search and the
// polynomial are ITS functions, compiled here for the device); engine side: table_engine.hpp.
//
// A byte mover with a table lookup in the middle: x is read once with 16-byte loads, T vectors are written with 16-byte stores, a
// grid-stride loop over groups of four elements with a capped grid; a lane's NEXT group is loaded before the current one is searched, so
// that a load is in flight during the search (the search is a chain of dependent LDS reads: without it the loop is latency).  A vector's storage is a multiple of 256 bytes (Pool::alloc rounds the
// capacity), so the last group is read and written whole: what lies past n is inside the buffer, and whatever value it holds finds a
// segment 0 … m like any other.
//
// Tables in LDS (dynamic, sized to the call: [coefficients T x (m + 1) x 32 B] [knots m x 8 B] [index (cells + 1) x 2 B], every part at
// a multiple of 16 bytes; 44 KiB at the most, a few hundred bytes for a short table, so that short tables keep the CU full).
// The search: a uniform grid of cells over [K[0], K[m−1]) gives the range of segments an element's cell can hold (fm_table_cell,
// fm_table_segment); uniform knots have at most one knot per cell — zero or one compare — and clustered knots are searched by bisection
// inside the cell; the end segments are found by two compares before the grid is asked.  The four coefficients of a segment are two
// 16-byte LDS reads per function.
// The kernel trusts its arguments: the launcher refuses what table_shape_ok refuses.  No register array is indexed at run time: no scratch.
#include <hip/hip_runtime.h>

#include "table_kernel.h"

namespace fm {

typedef float tb_f32x4 __attribute__((ext_vector_type(4)));
typedef tb_f32x4 __attribute__((address_space(1))) tb_gfloat4;

template <int T>
__global__ void __launch_bounds__(FM_TABLE_BLOCK) fm_table_apply_kernel(const DevTableArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char tb_lds[];
    const int m = (int)A.m, cells = (int)A.cells;
    double* C = reinterpret_cast<double*>(tb_lds);
    double* K = C + (size_t)T * (size_t)(m + 1) * 4;
    uint16_t* first = reinterpret_cast<uint16_t*>(K + m);
    for (int i = (int)threadIdx.x; i < T * (m + 1) * 4; i += FM_TABLE_BLOCK) C[i] = A.coefficients[i];
    for (int i = (int)threadIdx.x; i < m; i += FM_TABLE_BLOCK) K[i] = A.knots[i];
    for (int i = (int)threadIdx.x; i <= cells; i += FM_TABLE_BLOCK) first[i] = A.first[i];
    __syncthreads();
    const int64_t n = A.n;
    const double scale = A.scale, k_first = K[0], k_last = K[m - 1];
    const tb_gfloat4* __restrict__ px = reinterpret_cast<const tb_gfloat4*>(A.x);
    const int64_t stride = (int64_t)gridDim.x * FM_TABLE_BLOCK;
    int64_t i4 = (int64_t)blockIdx.x * FM_TABLE_BLOCK + threadIdx.x;
    tb_f32x4 ahead = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (i4 * 4 < n) ahead = px[i4];
#pragma unroll 1
    for (; i4 * 4 < n; i4 += stride) {
        const tb_f32x4 xv = ahead;
        if ((i4 + stride) * 4 < n) ahead = px[i4 + stride];          // the next group is on its way while this one is searched
        tb_f32x4 r[T];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double X = (double)xv[j];
            const int s = fmhost::fm_table_segment(K, m, first, cells, scale, X, k_first, k_last);
            const double a = K[s > 0 ? s - 1 : 0];
#pragma unroll
            for (int f = 0; f < T; ++f) r[f][j] = fmhost::fm_table_value(C + ((size_t)f * (size_t)(m + 1) + (size_t)s) * 4, X, a);
        }
#pragma unroll
        for (int f = 0; f < T; ++f) reinterpret_cast<tb_gfloat4*>(A.out[f])[i4] = r[f];
    }
}

hipError_t launch_table_apply(const DevTableArgs& a, hipStream_t st)
{
    if (!table_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(table_blocks(a.n)), block(FM_TABLE_BLOCK);
    const size_t lds = table_lds_bytes((int)a.m, (int)a.n_tables, (int)a.cells);
    switch (a.n_tables) {
    case 1: hipLaunchKernelGGL(fm_table_apply_kernel<1>, grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL(fm_table_apply_kernel<2>, grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL(fm_table_apply_kernel<3>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(fm_table_apply_kernel<4>, grid, block, lds, st, a); break;
    }
    return hipGetLastError();
}

} // namespace fm
