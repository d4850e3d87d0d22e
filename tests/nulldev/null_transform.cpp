// null_transform.cpp — TEST-ONLY stand-in for the launcher of transform_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  It refuses what the real launcher refuses (transform_shape_ok), reads the last
// 16-byte group of every operand and writes the last 16-byte group of every output the way the kernel does (a wild or undersized pointer is
// an ASan report), reads every row of the node table from the address the launch was given, and — device memory being host memory here —
// computes the results THE KERNEL'S WAY: group by group from the launch's own argument block, the node loop OUTSIDE the group's four
// elements, an element the definition closes early running through the nodes with k = 0, so that a wrong slot, scalar, address or row
// stride shows in what the driver compares with the definition.
#include <hip/hip_runtime_api.h>
#include <cstdint>

#include "../../finmath-lib-cuda-extensions_amd/csrc/transform_kernel.h"

namespace fm {

template <int S>
static void walk(const DevTransformArgs& a) {
    using namespace fmhost;
    const float* in[FM_TRANSFORM_OPERANDS];
    for (int k = 0; k < FM_TRANSFORM_OPERANDS; ++k) in[k] = k < 2 + S ? reinterpret_cast<const float*>((uintptr_t)a.in[k]) : nullptr;
    const int slot_delta = (int)(a.outputs & 1), slot_state = slot_delta + (int)((a.outputs >> 1) & 1);
    const int64_t groups = (a.n + 3) / 4;
    for (int64_t g = 0; g < groups; ++g) {                                                     // whole groups: the capacity is a multiple of 256 bytes
        double F[4], N[4], V0[4], V1[4], k[4];
        bool open[4];
        FmTransformOut closed[4];
        FmTransformSums sums[4];
        for (int e = 0; e < 4; ++e) {
            const int64_t p = g * 4 + e;
            F[e] = in[0] ? (double)in[0][p] : a.scalar[0]; N[e] = in[1] ? (double)in[1][p] : a.scalar[1];
            V0[e] = in[2] ? (double)in[2][p] : a.scalar[2]; V1[e] = in[3] ? (double)in[3][p] : a.scalar[3];
            k[e] = 0.0;
            closed[e].value = closed[e].delta = closed[e].state_delta = 0.0;
            open[e] = fm_transform_open(S, F[e], N[e], V0[e], V1[e], a.strike, k[e], closed[e]);
            sums[e].G = sums[e].H = sums[e].GV = 0.0;
        }
        for (uint32_t j = 0; j < a.n_nodes; ++j)
            for (int e = 0; e < 4; ++e) fm_transform_node<S>(a.nodes + (size_t)j * (3 + 2 * S), k[e], V0[e], V1[e], sums[e]);
        for (int e = 0; e < 4; ++e) {
            const int64_t p = g * 4 + e;
            const FmTransformOut r = open[e] ? fm_transform_close(F[e], N[e], a.strike, sums[e]) : closed[e];
            if (a.outputs & FM_TRANSFORM_VALUE) reinterpret_cast<float*>((uintptr_t)a.out[0])[p] = fm_narrow(r.value);
            if (a.outputs & FM_TRANSFORM_DELTA) reinterpret_cast<float*>((uintptr_t)a.out[slot_delta])[p] = fm_narrow(r.delta);
            if (a.outputs & FM_TRANSFORM_STATE_DELTA) reinterpret_cast<float*>((uintptr_t)a.out[slot_state])[p] = fm_narrow(r.state_delta);
        }
    }
}

hipError_t launch_transform_option(const DevTransformArgs& a, hipStream_t) {
    if (!transform_shape_ok(a)) return hipErrorInvalidValue;
    if (a.n_states == 0) walk<0>(a); else if (a.n_states == 1) walk<1>(a); else walk<2>(a);
    return hipSuccess;
}

} // namespace fm
