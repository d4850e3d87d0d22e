// kreg_engine.hpp — the engine's side of the kernel regression (kernel: kreg_kernel.hip; definition and argument check:
// host/kernel_regression.hpp).  Part of runtime.cpp's translation unit (included at its end behind side_pass_engine.hpp, nowhere else); a
// pass in that frame, as Engine::binned_xmom_pass is.
//
// kernel_moments_pass: the kernel-weighted local moments of up to 4 vectors at up to 256 points of a key vector from ONE launch: the
// arguments are checked by the function the host entry point uses before anything is flushed or launched, one flush, the vectors' storage
// held, lower / upper / points / rh go up in-stream, the wait under the engine lock, the sums come out of pinned memory.  Without the kernel
// the pass is FMHIP_ERR_UNSUPPORTED: the mirrors' host path is a caller's choice (FMHIP_DEVICE_KERNEL_MOMENTS=0), never the engine's.
#include "runtime.hpp"
#include "kreg_kernel.h"
#include "../host/kernel_regression.hpp"

#include <cstring>

namespace fm {

static_assert(FMHIP_KERNEL_UNIFORM == fmhost::FM_KERNEL_UNIFORM && FMHIP_KERNEL_TRIANGULAR == fmhost::FM_KERNEL_TRIANGULAR
              && FMHIP_KERNEL_EPANECHNIKOV == fmhost::FM_KERNEL_EPANECHNIKOV && FMHIP_KERNEL_QUARTIC == fmhost::FM_KERNEL_QUARTIC
              && FMHIP_KERNEL_TRIWEIGHT == fmhost::FM_KERNEL_TRIWEIGHT && FMHIP_KERNEL_MAX_POINTS == fmhost::FM_KERNEL_MAX_POINTS,
              "include/fmhip.h and host/kernel_regression.hpp name the same kernels");
static_assert(FM_KREG_MAX_POINTS == fmhost::FM_KERNEL_MAX_POINTS && FM_KREG_MAX_Y == fmhost::FM_KERNEL_MAX_Y
              && FM_KREG_MAX_ENTRIES_PER_POINT == fmhost::FM_KERNEL_MAX_ENTRIES_PER_POINT && FM_KREG_PAD == 2 * FM_KREG_MAX_POINTS,
              "kreg_kernel.h and host/kernel_regression.hpp describe the same pass");
static_assert((FM_KREG_MAX_POINTS + FM_KREG_ENTRIES / FM_KREG_MAX_ENTRIES_PER_POINT - 1) / (FM_KREG_ENTRIES / FM_KREG_MAX_ENTRIES_PER_POINT) <= FM_KREG_MAX_SLICES,
              "the widest call fits the slices");

// WEAK: see pass_need_kernel (tests/nulldev/null_kreg.cpp has the stand-in).
hipError_t launch_kernel_moments(const DevKernelMomentsArgs& a, hipStream_t st) __attribute__((weak));

void kernel_moments_check(fmhip_vec key, const double* points, const double* bandwidths, int n_points, int kernel, int order, const fmhip_vec* y, int n_y, const double* sums_out) {
    pass_as_engine_error([&] { fmhost::kernelMomentsCheck<fmhip_vec>(key, points, bandwidths, n_points, kernel, order, y, n_y, sums_out); });
}
// fmhip_kernel_moments_host: the definition, with its complaints as engine errors
void kernel_moments_host_checked(const float* key, int64_t n, const double* points, const double* bandwidths, int n_points, int kernel, int order, const float* const* y, int n_y, double* sums_out) {
    pass_as_engine_error([&] { fmhost::kernel_moments_host(key, n, points, bandwidths, n_points, kernel, order, y, n_y, sums_out); });
}

void Engine::kernel_moments_pass(fmhip_vec key, const double* points, const double* bandwidths, int n_points, int kernel, int order, const fmhip_vec* y, int n_y, double* sums_out) {
    require_init();
    kernel_moments_check(key, points, bandwidths, n_points, kernel, order, y, n_y, sums_out);
    fmhip_vec real[1 + FM_KREG_MAX_Y];
    int n_real = 0;
    real[n_real++] = key;
    for (int m = 0; m < n_y; ++m) real[n_real++] = y[m];
    pass_size(real, n_real, "kernel moments");
    pass_need_kernel(launch_kernel_moments != nullptr, "kernel-moments");
    PassHold hold;
    pass_prepare(real, n_real, hold, "kernel moments");
    DevKernelMomentsArgs a{};
    a.key = hold.ptrs[0];
    for (int m = 0; m < n_y; ++m) a.y[m] = hold.ptrs[(size_t)m + 1];
    const uint32_t Q = (uint32_t)n_points, qe = (uint32_t)fmhost::fm_kernel_entries(order, n_y);
    a.n_points = Q; a.kernel = (uint32_t)kernel; a.order = (uint32_t)order; a.n_y = (uint32_t)n_y;
    a.search_half = 1u;
    while (2u * a.search_half <= Q) a.search_half *= 2u;            // half the power of two above Q
    a.entries_per_point = qe;
    a.points_per_slice = std::min<uint32_t>(Q, (uint32_t)FM_KREG_ENTRIES / qe);
    a.n_slices = (Q + a.points_per_slice - 1) / a.points_per_slice;
    const uint32_t blocks = binned_blocks(hold.n);
    // pinned: [lower upper points rh (copied to the device in-stream)] [sums] [flag]; device: zero scratch = counters, other = tables + partials
    const size_t tab_bytes = pass_up256((size_t)4 * FM_KREG_MAX_POINTS * 8), out_bytes = pass_up256((size_t)Q * qe * 8);
    const size_t counters_bytes = pass_up256(((size_t)FM_KREG_MAX_SLICES + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + out_bytes + 64);
    pass_scratch(counters_bytes, tab_bytes + (size_t)a.n_slices * FM_KREG_ENTRIES * blocks * 8);
    double* tab = reinterpret_cast<double*>(stage);
    double* out_host = reinterpret_cast<double*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + out_bytes);
    a.counters = (uint32_t*)pass_zero_;
    a.n = hold.n; a.tiles = (uint32_t)((hold.n + FM_KREG_TILE - 1) / FM_KREG_TILE);
    a.tables = (const double*)pass_other_;
    a.partials = reinterpret_cast<double*>((char*)pass_other_ + tab_bytes);
    a.out_host = out_host;
    fmhost::kernel_edges(points, bandwidths, n_points, tab, tab + Q, tab + 3 * (size_t)Q);
    std::memcpy(tab + 2 * (size_t)Q, points, (size_t)Q * 8);
    hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(kernel points)");
    pass_launch(flag, a.done_flag, a.done_value, "kernel-moments pass", [&] { return launch_kernel_moments(a, stream_); });
    algorithmic_bytes_ += 4 * hold.n * (int64_t)n_real * (int64_t)a.n_slices;      // every slice reads the key and the y again
    std::memcpy(sums_out, out_host, (size_t)Q * qe * 8);
}

} // namespace fm
