// sobol_engine.hpp — the engine's side of the quasi-Monte-Carlo Brownian motion (definition: host/sobol.hpp; kernel:
// sobol_kernel.hip).  Part of runtime.cpp's translation unit (included at its end, nowhere else), like mt_generate_engine.hpp, whose pass
// this one is modelled on: the arguments are checked by the ONE function the host entry point uses (fmhost::sobolCheck) before anything is
// flushed or launched; the plan is built and validated on the host; the direction words of the dimensions in use, the digital shifts and
// the plan go up in one copy; the vectors are views into one slab of the pool, tagged as Brownian increments.  A Sobol' point is a function
// of its index, so a block of paths behind `path_offset` needs no prologue: one launch, whatever the offset.
// Which path a caller takes is the caller's choice (FMHIP_DEVICE_SOBOL=0 in the mirrors), never the engine's: without its kernel the pass
// is FMHIP_ERR_UNSUPPORTED; it never draws on the host.
#include "runtime.hpp"
#include "sobol_kernel.h"

#include <cstring>

namespace fm {

// WEAK, like the Mersenne-Twister launchers: a host-only build whose stand-in for the kernels does not know this one still links.
hipError_t launch_sobol_bm(const DevSobolArgs& a, hipStream_t st) __attribute__((weak));

// Everything that can be said about the arguments without a device, as an engine error
void sobol_check(int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, const fmhip_vec* out) {
    if (!out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "bad description of the Sobol' Brownian motion");
    try { fmhost::sobolCheck(randomize, construction, n_steps, n_factors, n_paths, path_offset, dt); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}

// fmhip_sobol_increments_host and fmhip_sobol_points_host: the definition, with its complaints as engine errors
void sobol_increments_host(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, double* host_out) {
    try { fmhost::sobolIncrements(seed, randomize, construction, n_steps, n_factors, n_paths, path_offset, dt, host_out); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}
void sobol_points_host(int n_dims, int64_t first_index, int64_t count, int32_t seed, int randomize, double* u_out) {
    try { fmhost::sobolPoints(n_dims, first_index, count, seed, randomize, u_out); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
}

void Engine::sobol_bm_generate(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out) {
    require_init();
    sobol_check(randomize, construction, n_steps, n_factors, n_paths, path_offset, dt, out);
    const int n_dims = n_steps * n_factors;
    fmhost::SobolPlan plan;
    try { plan = fmhost::sobolPlan(construction, n_steps, n_factors, dt); }
    catch (const std::invalid_argument& e) { throw Error(FMHIP_ERR_INVALID_ARGUMENT, e.what()); }
    if (!fmhost::sobolPlanOk(plan.ops.data(), plan.ops.size(), n_steps, n_factors, plan.n_slots)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "the plan of the Brownian bridge is inconsistent");
    if (launch_sobol_bm == nullptr) throw Error(FMHIP_ERR_UNSUPPORTED, "this build of the engine has no Sobol' kernel");
    // one block: plan (32 B per step) | direction words of the dimensions in use | shifts
    const size_t op_bytes = plan.ops.size() * sizeof(fmhost::SobolOp), dir_bytes = (size_t)n_dims * fmhost::FM_SOBOL_BITS * 4, shift_bytes = (size_t)n_dims * 4;
    const size_t bytes = op_bytes + dir_bytes + shift_bytes;
    int64_t stride = 0;
    Buffer* slab = slab_generate(n_paths, n_dims, &stride, [&](float* vectors) {
        void* dev = nullptr; size_t dev_cap = 0;
        try {
            char* st = (char*)ensure_stage(bytes);
            std::memcpy(st, plan.ops.data(), op_bytes);
            std::memcpy(st + op_bytes, fmhost::sobolDirections(), dir_bytes);
            const std::vector<uint32_t> shift = fmhost::sobolShifts(seed, randomize, n_dims);
            std::memcpy(st + op_bytes + dir_bytes, shift.data(), shift_bytes);
            dev = pool_.alloc(bytes, &dev_cap);
            hip_check(hipMemcpyAsync(dev, st, bytes, hipMemcpyHostToDevice, stream_), "Sobol' plan, direction numbers and shifts H2D");
            hip_check(hipStreamSynchronize(stream_), "sync");
            if (n_paths > 0) {
                DevSobolArgs a{};
                a.slab = vectors; a.stride_floats = stride;
                a.ops = reinterpret_cast<const fmhost::SobolOp*>(dev);
                a.directions = reinterpret_cast<const uint32_t*>((const char*)dev + op_bytes);
                a.shifts = reinterpret_cast<const uint32_t*>((const char*)dev + op_bytes + dir_bytes);
                a.n_paths = n_paths; a.path_offset = path_offset;
                a.n_ops = (uint32_t)plan.ops.size(); a.n_steps = (uint32_t)n_steps; a.n_factors = (uint32_t)n_factors; a.n_slots = (uint32_t)plan.n_slots;
                const int64_t first = path_offset + 1, last = path_offset + n_paths;
                a.first_block = (uint32_t)(first >> FM_SOBOL_BLOCK_LOG2);
                a.n_blocks = (uint32_t)((last >> FM_SOBOL_BLOCK_LOG2) - (first >> FM_SOBOL_BLOCK_LOG2) + 1);
                hip_check(launch_sobol_bm(a, stream_), "launch fm_sobol_bm_kernel");
                algorithmic_bytes_ += 4 * n_paths * n_dims;
                bytes_written_ += 4 * n_paths * n_dims;
                n_launches_++;
            }
        } catch (...) {
            if (dev) pool_.release(dev, dev_cap);
            throw;
        }
        pool_.release(dev, dev_cap);
    });
    slab_views(slab, stride, n_steps, n_factors, n_paths, out);
}

} // namespace fm
