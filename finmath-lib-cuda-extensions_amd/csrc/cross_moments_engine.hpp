// cross_moments_engine.hpp — the engine's side of the cross moments (kernel: fm_xmom_kernel in kernels.hip).  Part of
// runtime.cpp's translation unit (included at its end behind side_pass_engine.hpp, nowhere else).
//
// S[i][j] = Σ x_i·x_j (i <= j) and T[i][m] = Σ x_i·y_m of up to 12 + 4 vectors of one size in ONE launch: the normal equations of a
// least-squares regression, which the reference's callers assemble from K(K+3)/2 products and as many blocking averages
// (MonteCarloConditionalExpectationRegression: b_i.mult(b_j).getAverage()).  The pass stands in the frame of side_pass_engine.hpp: one
// flush, the vectors' storage held, one launch, the wait under the engine lock; then the sums are copied out of pinned memory.
#include "runtime.hpp"
#include "kernels.h"

#include <cstring>

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_xmom.cpp has the stand-in); the mirrors' generic path is a caller's choice
// (FMHIP_DEVICE_CROSS_MOMENTS=0), never the engine's.
hipError_t launch_xmom(const DevXmomArgs& a, hipStream_t st) __attribute__((weak));

// Everything that can be said about the arguments without looking at a vector
void xmom_check_counts(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, const double* sums_out) {
    if (n_x < 1 || n_x > FM_XMOM_MAX_X) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross moments of " + std::to_string(n_x) + " vectors: 1 … " + std::to_string(FM_XMOM_MAX_X));
    if (n_y < 0 || n_y > FM_XMOM_MAX_Y) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross moments with " + std::to_string(n_y) + " dependents: 0 … " + std::to_string(FM_XMOM_MAX_Y));
    if (!x || (n_y > 0 && !y) || !sums_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross moments: a required pointer is NULL");
    bool any = false;
    for (int i = 0; i < n_x; ++i) any |= x[i] != 0;
    if (!any) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross moments of the constant 1 alone have no size: at least one x is a vector");
    for (int m = 0; m < n_y; ++m) if (y[m] == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the constant 1 (handle 0) is an x, not a y");
}

void Engine::xmom_pass(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out) {
    require_init();
    xmom_check_counts(x, n_x, y, n_y, sums_out);
    // the list the kernel sees: x then y; `real` is the same without the ones, which is what has a node
    const int m = n_x + n_y;
    fmhip_vec list[FM_XMOM_MAX_X + FM_XMOM_MAX_Y], real[FM_XMOM_MAX_X + FM_XMOM_MAX_Y];
    int n_real = 0;
    for (int i = 0; i < m; ++i) { list[i] = i < n_x ? x[i] : y[i - n_x]; if (list[i]) real[n_real++] = list[i]; }
    pass_size(real, n_real, "cross moments");                // handles, sizes, n > 0: before anything is flushed or launched
    pass_need_kernel(launch_xmom != nullptr, "cross-moments");
    PassHold hold;
    pass_prepare(real, n_real, hold, "cross moments");
    DevXmomArgs a{};
    for (int i = 0, r = 0; i < m; ++i) a.vec[i] = list[i] ? hold.ptrs[(size_t)r++] : 0;
    // blocks of pairs of groups: (0,0); a second group adds (0,1), and (1,1) unless it holds dependents only
    a.n_blocks = 1;
    if (m > FM_XMOM_GROUP) {
        a.row_group[1] = 0; a.col_group[1] = 1; a.n_blocks = 2;
        if (n_x > FM_XMOM_GROUP) { a.row_group[2] = 1; a.col_group[2] = 1; a.n_blocks = 3; }
    }
    const uint32_t blocks = xmom_blocks(hold.n);
    const size_t out_bytes = pass_up256((size_t)FM_XMOM_MAX_BLOCKS * FM_XMOM_PAIRS * 8);
    char* stage = (char*)ensure_stage(out_bytes + 64);
    pass_scratch(pass_up256((FM_XMOM_MAX_BLOCKS + 1) * 4), (size_t)a.n_blocks * FM_XMOM_PAIRS * blocks * 8);
    double* out_host = reinterpret_cast<double*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + out_bytes);
    a.counters = (uint32_t*)pass_zero_;
    a.n = hold.n; a.tiles = (uint32_t)((hold.n + FM_XMOM_TILE - 1) / FM_XMOM_TILE);
    a.partials = (double*)pass_other_;
    a.out_host = out_host;
    pass_launch(flag, a.done_flag, a.done_value, "cross-moments pass", [&] { return launch_xmom(a, stream_); });
    auto entry = [&](int i, int j) {                         // i <= j in the list
        const int gi = i / FM_XMOM_GROUP, gj = j / FM_XMOM_GROUP;
        return out_host[(size_t)(gi + gj) * FM_XMOM_PAIRS + (size_t)(i % FM_XMOM_GROUP) * FM_XMOM_GROUP + (size_t)(j % FM_XMOM_GROUP)];
    };
    double* o = sums_out;
    for (int i = 0; i < n_x; ++i) for (int j = i; j < n_x; ++j) *o++ = entry(i, j);
    for (int i = 0; i < n_x; ++i) for (int k = 0; k < n_y; ++k) *o++ = entry(i, n_x + k);
}

} // namespace fm
