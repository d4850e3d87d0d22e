// side_pass_device.hpp — the tail every reducing side pass ends in, once: the arrival of the workgroups at a counter, the
// sum over the 64 lanes of a wave, and the combine of the workgroups' partials into pinned memory behind which the host's flag is raised.
// The device-side counterpart of side_pass_engine.hpp.  Only device code includes this; nothing of it goes to hiprtc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fm {

// The total of v over the 64 lanes of the wave, in every lane: the plain butterfly, bit 5 of the lane first.
__device__ __forceinline__ double pass_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Arrival counting at `counter` (zero before the launch, zero again after the last arrival): true, for the whole workgroup, in the LAST of
// `members` workgroups to arrive.  Whatever the others wrote before they arrived is visible to it: every thread's writes are released at
// agent scope before the barrier, the count is an agent-scope acquire-release add, and the last arriver's threads fence again behind the
// barrier (release, agent-scope add, acquire).  The reset by the last arriver is what lets the next launch of the stream find the counter
// at zero without a memset.  Every thread of the workgroup calls this, from uniform control flow: it holds two barriers, and its flag is ONE
// word of LDS however many calls a kernel makes.
__device__ __forceinline__ bool pass_arrive_last(uint32_t* counter, const uint32_t members)
{
    __shared__ uint32_t last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t arrived = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = (arrived == members - 1u) ? 1u : 0u;
        if (last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const bool r = last != 0u;
    if (r) __threadfence();
    return r;
}

struct PassNothingElse { __device__ __forceinline__ void operator()() const {} };

// The end of a pass whose grid is (workgroups of a slice, slices), for a workgroup of BLOCK threads that holds, in LDS, BLOCK / 64 per-wave
// partials of each of its `used` (<= BLOCK) entries: wave w's partial of entry e is wave_part[w * wave_stride + e], written before a barrier.
//   part            this slice's [entry][gridDim.x] block of device scratch
//   out             this slice's first entry in pinned host memory
//   slice_counter   this slice's arrival counter; launch_counter the one the slices share (both zero before, zero again after)
//   also            what else the last workgroup of the slice moves to pinned memory, run between the sums and the system-scope fence
// Order of the additions of one entry: the waves of a workgroup in order; the workgroups' partials lane-strided by one wave of the last
// workgroup of the slice to arrive, then the butterfly — a function of gridDim.x alone.  Behind the system-scope fence the slice is counted
// across gridDim.y, and the last slice's last workgroup stores done_value to the host's flag (system-scope release).
template <int BLOCK, class Also = PassNothingElse>
__device__ __forceinline__ void pass_combine_partials(const double* wave_part, const uint32_t wave_stride, const uint32_t used, double* part, double* out,
                                                      uint32_t* slice_counter, uint32_t* launch_counter, uint64_t* done_flag, const uint64_t done_value,
                                                      Also also = Also())
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < used) {
        double s = wave_part[tid];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) s += wave_part[(uint32_t)w * wave_stride + tid];
        part[(size_t)tid * gridDim.x + blockIdx.x] = s;
    }
    if (!pass_arrive_last(slice_counter, gridDim.x)) return;
    for (uint32_t e = tid >> 6; e < used; e += BLOCK / 64) {
        double s = 0.0;
        for (uint32_t b = lane; b < gridDim.x; b += 64u) s += part[(size_t)e * gridDim.x + b];
        s = pass_wave_sum(s);
        if (lane == 0u) out[e] = s;
    }
    also();
    __threadfence_system();
    if (!pass_arrive_last(launch_counter, gridDim.y)) return;
    if (tid == 0u) __hip_atomic_store(done_flag, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

} // namespace fm
