// null_implied_volatility.cpp — TEST-ONLY stand-in for the launcher of implied_volatility_kernel.hip, beside the null device of tests/nulldev
// (null_hip.cpp: device memory is host memory, launches compute nothing).  It refuses what the real launcher refuses (implied_shape_ok),
// reads the last 16-byte group of every operand and writes the last 16-byte group of every output the way the kernel does (a wild or
// undersized pointer is an ASan report), and — device memory being host memory here — computes the results THE KERNEL'S WAY: group by group
// from the launch's own argument block (mask, output slots, operands that are a vector or a scalar), so that a wrong slot, scalar or address
// shows in what the driver compares with the definition.
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../finmath-lib-cuda-extensions_amd/csrc/implied_volatility_kernel.h"

namespace fm {

hipError_t launch_implied_volatility(const DevImpliedArgs& a, hipStream_t) {
    if (!implied_shape_ok(a)) return hipErrorInvalidValue;
    const float* in[3];
    for (int k = 0; k < 3; ++k) in[k] = reinterpret_cast<const float*>((uintptr_t)a.in[k]);
    const int slot_d_price = (int)(a.outputs & 1), slot_d_forward = slot_d_price + (int)((a.outputs >> 1) & 1);
    const bool partials = (a.outputs & (fmhost::FM_IMPLIED_D_PRICE | fmhost::FM_IMPLIED_D_FORWARD)) != 0;
    const int64_t groups = (a.n + 3) / 4;
    for (int64_t g = 0; g < groups; ++g)                                                       // whole groups: the capacity is a multiple of 256 bytes
        for (int j = 0; j < 4; ++j) {
            const int64_t p = g * 4 + j;
            const fmhost::FmImpliedOut r = fmhost::fm_implied_volatility_masked((int)a.model, in[0] ? (double)in[0][p] : a.scalar[0], in[1] ? (double)in[1][p] : a.scalar[1],
                                                                                in[2] ? (double)in[2][p] : a.scalar[2], a.root_T, a.strike, partials);
            if (a.outputs & fmhost::FM_IMPLIED_VOLATILITY) reinterpret_cast<float*>((uintptr_t)a.out[0])[p] = fmhost::fm_narrow(r.sigma);
            if (a.outputs & fmhost::FM_IMPLIED_D_PRICE) reinterpret_cast<float*>((uintptr_t)a.out[slot_d_price])[p] = fmhost::fm_narrow(r.d_price);
            if (a.outputs & fmhost::FM_IMPLIED_D_FORWARD) reinterpret_cast<float*>((uintptr_t)a.out[slot_d_forward])[p] = fmhost::fm_narrow(r.d_forward);
        }
    return hipSuccess;
}

} // namespace fm
