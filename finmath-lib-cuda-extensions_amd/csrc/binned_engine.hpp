// binned_engine.hpp — the engine's side of the localized regression (kernels: binned_kernel.hip; definition and argument
// checks: host/binned_regression.hpp).  Passes in the frame of side_pass_engine.hpp (which says what every such pass does): the first a
// reducing one, as the cross moments are, the second a producing one.
//
// binned_xmom_pass: the count and the cross moments of up to 3 + 4 vectors PER BIN of a key vector — the block-diagonal normal equations of
// a regression that is local in the key — from ONE launch.
// binned_eval: the piecewise estimate as a new vector: the bounds and the narrowed coefficients go up in one copy that the host waits for
// (the pinned staging block is the engine's: it must be free again when the call returns); the launch itself is not waited for.
#include "runtime.hpp"
#include "binned_kernel.h"
#include "../host/binned_regression.hpp"

#include <cstring>

namespace fm {

static_assert(FM_BINNED_MAX_BINS == fmhost::FM_BINNED_MAX_BINS && FM_BINNED_MAX_X == fmhost::FM_BINNED_MAX_X && FM_BINNED_MAX_Y == fmhost::FM_BINNED_MAX_Y,
              "binned_kernel.h and host/binned_regression.hpp describe the same passes");

// WEAK: see pass_need_kernel (tests/nulldev/null_binned.cpp has the stand-ins).
hipError_t launch_binned_xmom(const DevBinnedXmomArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_binned_eval(const DevBinnedEvalArgs& a, hipStream_t st) __attribute__((weak));

void binned_check_moments(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, const int64_t* counts_out, const double* sums_out) {
    pass_as_engine_error([&] { fmhost::binnedCheckMoments<fmhip_vec>(key, bounds, n_bins, x, n_x, y, n_y, counts_out, sums_out); });
}
void binned_check_evaluate(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const double* coefficients, const fmhip_vec* out) {
    pass_as_engine_error([&] { fmhost::binnedCheckEvaluate<fmhip_vec>(key, bounds, n_bins, x, n_x, coefficients, out); });
}
// fmhip_binned_cross_moments_host and fmhip_binned_evaluate_host: the definition, with its complaints as engine errors
void binned_cross_moments_host(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x, const float* const* y, int n_y, int64_t* counts_out, double* sums_out) {
    pass_as_engine_error([&] { fmhost::binnedCrossMoments(key, n, bounds, n_bins, x, n_x, y, n_y, counts_out, sums_out); });
}
void binned_evaluate_host(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x, const double* coefficients, float* out) {
    pass_as_engine_error([&] { fmhost::binnedEvaluate(key, n, bounds, n_bins, x, n_x, coefficients, out); });
}

// key first, then the vectors among x and y: handles, one size, n > 0 — before anything is flushed or launched
static int binned_real(Engine& e, fmhip_vec key, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, fmhip_vec* real, const char* what) {
    int n_real = 0;
    real[n_real++] = key;
    for (int i = 0; i < n_x; ++i) if (x[i]) real[n_real++] = x[i];
    for (int m = 0; m < n_y; ++m) real[n_real++] = y[m];
    e.pass_size(real, n_real, what);
    return n_real;
}

void Engine::binned_xmom_pass(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, int64_t* counts_out, double* sums_out) {
    require_init();
    binned_check_moments(key, bounds, n_bins, x, n_x, y, n_y, counts_out, sums_out);
    fmhip_vec real[1 + FM_BINNED_MAX_X + FM_BINNED_MAX_Y];
    const int n_real = binned_real(*this, key, x, n_x, y, n_y, real, "binned cross moments");
    pass_need_kernel(launch_binned_xmom != nullptr, "binned cross-moments");
    PassHold hold;
    pass_prepare(real, n_real, hold, "binned cross moments");
    DevBinnedXmomArgs a{};
    int r = 0;
    a.key = hold.ptrs[(size_t)r++];
    for (int i = 0; i < n_x; ++i) a.x[i] = x[i] ? hold.ptrs[(size_t)r++] : 0;
    for (int m = 0; m < n_y; ++m) a.y[m] = hold.ptrs[(size_t)r++];
    // the products the call asks for, as entries of a bin; the product of two constants is the bin's count and takes no entry
    auto s_slot = [](int i, int c) { return i * FM_BINNED_MAX_X - i * (i - 1) / 2 + (c - i); };
    auto t_slot = [](int i, int m) { return FM_BINNED_MAX_X * (FM_BINNED_MAX_X + 1) / 2 + i * FM_BINNED_MAX_Y + m; };
    for (int s = 0; s < FM_BINNED_SLOTS + 2; ++s) a.slot_entry[s] = -1;
    int qe = 0;
    for (int i = 0; i < n_x; ++i) for (int c = i; c < n_x; ++c) if (x[i] || x[c]) a.slot_entry[s_slot(i, c)] = (int8_t)qe++;
    for (int i = 0; i < n_x; ++i) for (int m = 0; m < n_y; ++m) a.slot_entry[t_slot(i, m)] = (int8_t)qe++;
    if (qe == 0) a.slot_entry[s_slot(0, 0)] = (int8_t)qe++;      // constants alone: the counts are all there is, the kernel still wants an entry
    a.n_bins = (uint32_t)n_bins; a.n_x = (uint32_t)n_x; a.n_y = (uint32_t)n_y;
    a.entries_per_bin = (uint32_t)qe;
    a.bins_per_slice = std::min<uint32_t>((uint32_t)n_bins, (uint32_t)FM_BINNED_ENTRIES / (uint32_t)qe);
    a.n_slices = (a.n_bins + a.bins_per_slice - 1) / a.bins_per_slice;
    const uint32_t blocks = binned_blocks(hold.n);
    // pinned: [bounds (copied to the device in-stream)] [sums] [counts] [flag]; device: zero scratch = counters + counts, other = bounds + partials
    const size_t tab_bytes = pass_up256((size_t)FM_BINNED_MAX_BINS * 8), out_bytes = pass_up256((size_t)n_bins * qe * 8), cnt_bytes = pass_up256((size_t)FM_BINNED_MAX_BINS * 4);
    const size_t counters_bytes = pass_up256(((size_t)FM_BINNED_MAX_SLICES + 1) * 4);
    char* stage = (char*)ensure_stage(tab_bytes + out_bytes + cnt_bytes + 64);
    pass_scratch(counters_bytes + cnt_bytes, tab_bytes + (size_t)a.n_slices * FM_BINNED_ENTRIES * blocks * 8);
    double* out_host = reinterpret_cast<double*>(stage + tab_bytes);
    uint32_t* counts_host = reinterpret_cast<uint32_t*>(stage + tab_bytes + out_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + out_bytes + cnt_bytes);
    a.counters = (uint32_t*)pass_zero_;
    a.counts_dev = reinterpret_cast<uint32_t*>((char*)pass_zero_ + counters_bytes);
    a.n = hold.n; a.tiles = (uint32_t)((hold.n + FM_BINNED_TILE - 1) / FM_BINNED_TILE);
    a.bounds = (const double*)pass_other_;
    a.partials = reinterpret_cast<double*>((char*)pass_other_ + tab_bytes);
    a.out_host = out_host; a.counts_host = counts_host;
    if (n_bins > 1) {
        std::memcpy(stage, bounds, (size_t)(n_bins - 1) * 8);
        hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(bin bounds)");
    }
    pass_launch(flag, a.done_flag, a.done_value, "binned cross-moments pass", [&] { return launch_binned_xmom(a, stream_); });
    const int q = fmhost::binnedSumsPerBin(n_x, n_y);
    for (int b = 0; b < n_bins; ++b) {
        counts_out[b] = (int64_t)counts_host[b];
        double* o = sums_out + (size_t)b * q;
        auto entry = [&](int slot) { const int e = a.slot_entry[slot]; return e >= 0 ? out_host[(size_t)b * qe + e] : (double)counts_host[b]; };
        for (int i = 0; i < n_x; ++i) for (int c = i; c < n_x; ++c) *o++ = entry(s_slot(i, c));
        for (int i = 0; i < n_x; ++i) for (int m = 0; m < n_y; ++m) *o++ = entry(t_slot(i, m));
    }
}

void Engine::binned_eval(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const double* coefficients, fmhip_vec* out) {
    require_init();
    binned_check_evaluate(key, bounds, n_bins, x, n_x, coefficients, out);
    fmhip_vec real[1 + FM_BINNED_MAX_X];
    const int n_real = binned_real(*this, key, x, n_x, nullptr, 0, real, "binned evaluation");
    pass_need_kernel(launch_binned_eval != nullptr, "binned evaluation");
    PassHold hold;
    pass_prepare(real, n_real, hold, "binned evaluation");
    DevBinnedEvalArgs a{};
    int r = 0;
    a.key = hold.ptrs[(size_t)r++];
    for (int i = 0; i < n_x; ++i) a.x[i] = x[i] ? hold.ptrs[(size_t)r++] : 0;
    a.n = hold.n; a.n_bins = (uint32_t)n_bins; a.n_x = (uint32_t)n_x;
    PassOutputs outs(this);
    a.out = outs.add(hold.n);
    // bounds and the coefficients narrowed to fp32 go up in one copy; the copy has left the pinned block before this call returns
    const size_t tab_bytes = pass_up256((size_t)FM_BINNED_MAX_BINS * 8), coef_bytes = pass_up256((size_t)FM_BINNED_MAX_BINS * FM_BINNED_MAX_X * 4);
    char* stage = (char*)ensure_stage(tab_bytes + coef_bytes);
    pass_scratch(pass_up256(8), tab_bytes + coef_bytes);
    std::memset(stage, 0, tab_bytes + coef_bytes);
    if (n_bins > 1) std::memcpy(stage, bounds, (size_t)(n_bins - 1) * 8);
    float* c = reinterpret_cast<float*>(stage + tab_bytes);
    for (int i = 0; i < n_bins * n_x; ++i) c[i] = (float)coefficients[i];
    hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes + coef_bytes, hipMemcpyHostToDevice, stream_), "H2D(bin bounds and coefficients)");
    hip_check(hipStreamSynchronize(stream_), "sync");
    a.bounds = (const double*)pass_other_;
    a.coefficients = reinterpret_cast<const float*>((const char*)pass_other_ + tab_bytes);
    hip_check(launch_binned_eval(a, stream_), "launch fm_binned_eval_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (n_real + 1);
    bytes_written_ += 4 * hold.n;
    outs.commit(out);
}

} // namespace fm
