// table_engine.hpp — the engine's side of the tabulated functions (kernel: table_kernel.hip; definition, index and argument
// checks: host/tabulated_function.hpp).  A producing pass in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// table_apply: up to four functions on the same knots applied to every element of x, each result a new vector.  The knots, the coefficients
// and the coarse index go up in ONE in-stream copy from the pinned stage that the host waits for (the staging block is the engine's: it
// must be free again when the call returns); the launch itself is not waited for — as Engine::binned_eval.  The pass is elementwise: a
// device list runs it per shard (sharded.cpp), a communicator's ranks each on their own paths.
#include "runtime.hpp"
#include "table_kernel.h"

#include <cstring>

namespace fm {

static_assert(FMHIP_TABLE_PIECEWISE_CONSTANT == fmhost::FM_TABLE_PIECEWISE_CONSTANT && FMHIP_TABLE_LINEAR == fmhost::FM_TABLE_LINEAR
              && FMHIP_TABLE_CUBIC_SPLINE == fmhost::FM_TABLE_CUBIC_SPLINE && FMHIP_TABLE_MONOTONE_CUBIC == fmhost::FM_TABLE_MONOTONE_CUBIC
              && FMHIP_TABLE_CONSTANT == fmhost::FM_TABLE_CONSTANT && FMHIP_TABLE_LINEAR_EXTRAPOLATION == fmhost::FM_TABLE_LINEAR_EXTRAPOLATION
              && FMHIP_TABLE_MAX_KNOTS == fmhost::FM_TABLE_MAX_KNOTS, "include/fmhip.h and host/tabulated_function.hpp name the same modes");

// WEAK: see pass_need_kernel (tests/nulldev/null_table.cpp has the stand-in).
hipError_t launch_table_apply(const DevTableArgs& a, hipStream_t st) __attribute__((weak));

void table_check_apply(fmhip_vec x, const double* knots, int count, const double* coefficients, int n_tables, const fmhip_vec* out) {
    if (!x) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "tabulated function: of a vector");
    pass_as_engine_error([&] { fmhost::tableCheckApply(knots, count, coefficients, n_tables, out); });
}
// fmhip_table_build and fmhip_table_apply_host: the definition, with its complaints as engine errors
void table_build_checked(const double* knots, const double* values, int count, int interpolation, int extrapolation, int derivative, double* coefficients_out) {
    pass_as_engine_error([&] { fmhost::table_build(knots, values, count, interpolation, extrapolation, derivative, coefficients_out); });
}
void table_apply_host_checked(const float* x, int64_t n, const double* knots, int count, const double* coefficients, int n_tables, float* const* out) {
    pass_as_engine_error([&] { fmhost::table_apply_host(x, n, knots, count, coefficients, n_tables, out); });
}

void Engine::table_apply(fmhip_vec x, const double* knots, int count, const double* coefficients, int n_tables, fmhip_vec* out) {
    require_init();
    table_check_apply(x, knots, count, coefficients, n_tables, out);
    pass_size(&x, 1, "tabulated function");
    pass_need_kernel(launch_table_apply != nullptr, "tabulated-function");
    PassHold hold;
    pass_prepare(&x, 1, hold, "tabulated function");
    const int cells = fmhost::fm_table_cells(count);
    DevTableArgs a{};
    a.n = hold.n; a.m = (uint32_t)count; a.n_tables = (uint32_t)n_tables; a.cells = (uint32_t)cells;
    a.x = hold.ptrs[0];
    PassOutputs outs(this);
    for (int f = 0; f < n_tables; ++f) a.out[f] = outs.add(hold.n);
    // knots, coefficients and index go up in one copy; the copy has left the pinned block before this call returns
    const size_t k_bytes = table_knots_bytes(count), c_bytes = table_coefficients_bytes(count, n_tables), all_bytes = table_block_bytes(count, n_tables, cells);
    char* stage = (char*)ensure_stage(all_bytes);
    pass_scratch(pass_up256(8), all_bytes);
    std::memset(stage, 0, all_bytes);
    std::memcpy(stage, knots, (size_t)count * 8);
    std::memcpy(stage + k_bytes, coefficients, (size_t)n_tables * (size_t)(count + 1) * 32);
    fmhost::table_index_build(knots, count, cells, &a.scale, reinterpret_cast<uint16_t*>(stage + k_bytes + c_bytes));
    hip_check(hipMemcpyAsync(pass_other_, stage, all_bytes, hipMemcpyHostToDevice, stream_), "H2D(knots, coefficients and index)");
    hip_check(hipStreamSynchronize(stream_), "sync");
    a.knots = (const double*)pass_other_;
    a.coefficients = reinterpret_cast<const double*>((const char*)pass_other_ + k_bytes);
    a.first = reinterpret_cast<const uint16_t*>((const char*)pass_other_ + k_bytes + c_bytes);
    hip_check(launch_table_apply(a, stream_), "launch fm_table_apply_kernel");
    ++n_launches_;
    algorithmic_bytes_ += 4 * hold.n * (1 + n_tables);
    bytes_written_ += 4 * hold.n * n_tables;
    outs.commit(out);
}

} // namespace fm
