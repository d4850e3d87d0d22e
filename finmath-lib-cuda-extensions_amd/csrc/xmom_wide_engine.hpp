// xmom_wide_engine.hpp — the engine's side of the wide cross moments (kernel: fm_xmom_wide_kernel in xmom_wide_kernel.hip).
// Part of runtime.cpp's translation unit (included at its end behind side_pass_engine.hpp, nowhere else).
//
// S[i][j] = Σ x_i·x_j (i <= j) and T[i][m] = Σ x_i·y_m of up to 64 vectors of one size in ONE launch on the matrix cores: the normal
// equations of a regression on more basis functions than cross_moments_engine.hpp's register file holds.  Layout, the constant 1, status
// codes and IEEE behaviour are fmhip_cross_moments'; the bits are this pass's own (another tree).  The pass stands in the frame of
// side_pass_engine.hpp: one flush, the vectors' storage held, one launch, the wait under the engine lock; then the sums are copied out of
// pinned memory.
#include "runtime.hpp"
#include "xmom_wide_kernel.h"

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_xmom_wide.cpp has the stand-in); the mirrors' pair-by-pair path is a caller's choice
// (FMHIP_DEVICE_WIDE_MOMENTS=0), never the engine's.
hipError_t launch_xmom_wide(const DevXmomWideArgs& a, hipStream_t st) __attribute__((weak));

// Everything that can be said about the arguments without looking at a vector
void xmom_wide_check_counts(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, const double* sums_out) {
    if (n_x < 1 || n_y < 0 || n_x > FM_XMOMW_MAX || n_y > FM_XMOMW_MAX || n_x + n_y > FM_XMOMW_MAX)
        throw Error(FMHIP_ERR_INVALID_ARGUMENT, "wide cross moments of " + std::to_string(n_x) + " + " + std::to_string(n_y) + " vectors: n_x >= 1, n_y >= 0, n_x + n_y <= " + std::to_string(FM_XMOMW_MAX));
    if (!x || (n_y > 0 && !y) || !sums_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "wide cross moments: a required pointer is NULL");
    bool any = false;
    for (int i = 0; i < n_x; ++i) any |= x[i] != 0;
    if (!any) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "cross moments of the constant 1 alone have no size: at least one x is a vector");
    for (int m = 0; m < n_y; ++m) if (y[m] == 0) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the constant 1 (handle 0) is an x, not a y");
}

void Engine::xmom_wide_pass(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out) {
    require_init();
    xmom_wide_check_counts(x, n_x, y, n_y, sums_out);
    // the list the kernel sees: x then y; `real` is the same without the ones, which is what has a node
    const int m = n_x + n_y;
    fmhip_vec list[FM_XMOMW_MAX], real[FM_XMOMW_MAX];
    int n_real = 0;
    for (int i = 0; i < m; ++i) { list[i] = i < n_x ? x[i] : y[i - n_x]; if (list[i]) real[n_real++] = list[i]; }
    pass_size(real, n_real, "wide cross moments");           // handles, sizes, n > 0: before anything is flushed or launched
    pass_need_kernel(launch_xmom_wide != nullptr, "wide cross-moments");
    PassHold hold;
    pass_prepare(real, n_real, hold, "wide cross moments");
    // pinned: [sums] [flag]
    const size_t out_bytes = pass_up256((size_t)FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES * 8);
    char* stage = (char*)ensure_stage(out_bytes + 64);
    DevXmomWideArgs a{};
    for (int i = 0, r = 0; i < FM_XMOMW_MAX; ++i) a.vec[i] = i >= m ? FM_XMOMW_PAD : list[i] ? hold.ptrs[(size_t)r++] : FM_XMOMW_ONE;
    const uint32_t blocks = xmom_wide_blocks(hold.n);
    pass_scratch(256, (size_t)blocks * FM_XMOMW_MAX_TILES * FM_XMOMW_TILE_ENTRIES * 8);
    double* out_host = reinterpret_cast<double*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + out_bytes);
    a.counter = (uint32_t*)pass_zero_;
    a.n = hold.n; a.chunks = (uint32_t)((hold.n + FM_XMOMW_CHUNK - 1) / FM_XMOMW_CHUNK);
    a.n_groups = (uint32_t)((m + FM_XMOMW_GROUP - 1) / FM_XMOMW_GROUP);
    a.partials = (double*)pass_other_;
    a.out_host = out_host;
    pass_launch(flag, a.done_flag, a.done_value, "wide cross-moments pass", [&] { return launch_xmom_wide(a, stream_); });
    double* o = sums_out;
    for (int i = 0; i < n_x; ++i) for (int j = i; j < n_x; ++j) *o++ = out_host[xmom_wide_entry(i, j)];
    for (int i = 0; i < n_x; ++i) for (int k = 0; k < n_y; ++k) *o++ = out_host[xmom_wide_entry(i, n_x + k)];
}

} // namespace fm
