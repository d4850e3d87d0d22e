// null_xmom_poly.cpp — TEST-ONLY stand-ins for the launchers of xmom_poly_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp:
// device memory is host memory, launches compute nothing).  The first and last element of the scratch the moments launch is handed are
// touched (a wild or undersized pointer is an ASan report), and — device memory being host memory here — both stand-ins compute the host
// DEFINITION (host/polynomial_regression.hpp) from the launch arguments: the sums stored where xmom_wide_entry says, the fitted polynomial
// written to the new vector's storage, so the driver checks the slots, the layout and the shard sums on the entries whose values it knows;
// the completion flag is raised.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/xmom_poly_kernel.h"
#include "../../finmath-lib-cuda-extensions_amd/host/polynomial_regression.hpp"

namespace fm {

hipError_t launch_xmom_poly(const DevXmomPolyArgs& p, hipStream_t) {
    if (!xmom_poly_shape_ok(p)) return hipErrorInvalidValue;
    const DevXmomWideArgs& a = p.w;
    if (*(volatile uint32_t*)a.counter != 0u) return hipErrorInvalidValue;                 // zero between launches
    const size_t per_block = (size_t)FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES;
    a.partials[0] = 0.0;
    a.partials[(size_t)xmom_wide_blocks(a.n) * per_block - 1] = 0.0;
    const int m = (int)a.n_groups * FM_XMOMW_GROUP;
    auto at = [&](int i, int64_t path) {
        const uint64_t slot = a.vec[i];
        if (slot == FM_XMOMW_ONE) return 1.0;
        if (slot == FM_XMOMW_PAD) return 0.0;
        if (slot & FM_XMOMW_TERM) {
            float u[FM_POLY_MAX_STATES]; uint8_t e[FM_POLY_MAX_STATES];
            for (uint32_t s = 0; s < p.n_states; ++s) { u[s] = reinterpret_cast<const float*>((uintptr_t)p.state[s])[path]; e[s] = (uint8_t)((slot >> (3 * s)) & 7u); }
            return (double)fmhost::polynomialTerm(u, (int)p.n_states, e);
        }
        return (double)reinterpret_cast<const float*>((uintptr_t)slot)[path];
    };
    for (int i = 0; i < m; ++i)
        for (int j = i; j < m; ++j) {
            double s = 0.0;
            for (int64_t path = 0; path < a.n; ++path) s += at(i, path) * at(j, path);
            a.out_host[xmom_wide_entry(i, j)] = s;
        }
    __atomic_store_n(a.done_flag, a.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

hipError_t launch_poly_eval(const DevPolyEvalArgs& a, hipStream_t) {
    if (!poly_eval_shape_ok(a)) return hipErrorInvalidValue;
    std::vector<const float*> states, extra;
    std::vector<uint8_t> e;
    std::vector<double> c;
    for (uint32_t s = 0; s < a.n_states; ++s) states.push_back(reinterpret_cast<const float*>((uintptr_t)a.state[s]));
    for (uint32_t i = 0; i < a.n_terms; ++i) for (uint32_t s = 0; s < a.n_states; ++s) e.push_back((uint8_t)((a.exponents[i] >> (3 * s)) & 7u));
    for (uint32_t j = 0; j < a.n_extra; ++j) extra.push_back(reinterpret_cast<const float*>((uintptr_t)a.extra[j]));
    for (uint32_t i = 0; i < a.n_terms + a.n_extra; ++i) c.push_back((double)a.coefficient[i]);
    fmhost::polynomialEvaluate(states.data(), a.n, (int)a.n_states, e.data(), (int)a.n_terms, a.n_extra ? extra.data() : nullptr, (int)a.n_extra, c.data(), reinterpret_cast<float*>((uintptr_t)a.out));
    return hipSuccess;
}

} // namespace fm
