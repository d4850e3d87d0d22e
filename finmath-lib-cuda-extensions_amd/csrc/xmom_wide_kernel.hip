// xmom_wide_kernel.hip — fm_xmom_wide_kernel for gfx950 (MI355X, CDNA4): the normal equations of a least-squares regression on up to 64
// vectors — XᵀX — in one pass, on the matrix cores.  DESIGN.md §4.14; contract: include/fmhip.h; layout, tree and L(n): xmom_wide_kernel.h;
// engine side: xmom_wide_engine.hpp.
//
// v_mfma_f64_16x16x4_f64 computes D = A·B + C for a 16 x 4 A, a 4 x 16 B and a 16 x 16 C/D.  Lane l holds ONE f64 of A, A[l & 15][l >> 4], and
// one of B, B[l >> 4][l & 15]; C/D are 4 f64 per lane, col = l & 15, row = (l >> 4) + 4·reg (this is NOT the f32 forms' row formula).
// With rows of A = vectors of group g, columns of B = vectors of group h and k = a path, lane l needs x_{16g + (l & 15)} at path p + (l >> 4)
// as the A operand of group g AND as the B operand of group g: one register serves both, no transpose, no LDS staging, no second load.
//
// Loads.  A wave takes a chunk of 64 paths: per group four 16-byte loads per lane, load r from vector (l & 15) at path 16r + 4·(l >> 4).  The
// four floats of a load feed four MFMA steps; step s sums over the paths 16r + 4k + s, k = 0 … 3 — both operands use the same path-to-k
// map, which is all that correctness asks.  The wave reads whole 256-byte lines of every vector, and a round's loads are issued before
// the MFMAs of the round before it.  A vector's storage is padded to 256 bytes, so every chunk that starts below n is in bounds; paths past
// n are +0.0 in both operands, the constant 1 included.
//
// A product of two fp32 values is exact in fp64, so every step adds exact products; what rounds is the running sum.  No fp32 product, no
// float atomics.  The tree is in xmom_wide_kernel.h; its code, shared with fm_xmom_poly_kernel, in xmom_wide_device.hpp.  The kernel trusts its arguments: the launcher refuses what xmom_wide_shape_ok
// refuses.  No register array is indexed at run time: no scratch.
#include <hip/hip_runtime.h>

#include "xmom_wide_device.hpp"

namespace fm {

// every slot is an address, the constant 1 or a zero operand; the tail is zeroed as the loads arrive
template <int NG>
struct XwWidePolicy {
    typedef XwRound<NG> Raw;
    XwAddressLoads<NG, false> a;
    int64_t n;
    uint32_t sub;
    __device__ __forceinline__ void init(const uint64_t* slots, const uint32_t lane, const uint32_t sub_) { sub = sub_; a.init(slots, lane, sub_); }
    __device__ __forceinline__ void load(const uint32_t c, const int r, Raw& k) const
    {
        a.load(c, r, k);
        xw_zero_tail<NG>(k, (int64_t)c * FM_XMOMW_CHUNK + r * 16 + sub * 4u, n);
    }
    __device__ __forceinline__ void form(uint32_t, int, const Raw& k, XwRound<NG>& o) const { o = k; }
};

template <int NG>
__global__ void __launch_bounds__(FM_XMOMW_BLOCK) fm_xmom_wide_kernel(const DevXmomWideArgs A)
{
    XwWidePolicy<NG> P;
    P.n = A.n;
    xw_pass<NG>(A, P);
}

hipError_t launch_xmom_wide(const DevXmomWideArgs& a, hipStream_t st)
{
    if (!xmom_wide_shape_ok(a)) return hipErrorInvalidValue;
    const dim3 grid(xmom_wide_blocks(a.n), 1, 1), block(FM_XMOMW_BLOCK);
    switch (a.n_groups) {
    case 1:  hipLaunchKernelGGL(fm_xmom_wide_kernel<1>, grid, block, 0, st, a); break;
    case 2:  hipLaunchKernelGGL(fm_xmom_wide_kernel<2>, grid, block, 0, st, a); break;
    case 3:  hipLaunchKernelGGL(fm_xmom_wide_kernel<3>, grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL(fm_xmom_wide_kernel<4>, grid, block, 0, st, a); break;
    }
    return hipGetLastError();
}

} // namespace fm
