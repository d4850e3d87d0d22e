// null_os.cpp — TEST-ONLY stand-ins for the three order-statistics launchers of kernels.hip, beside the null device of tests/nulldev
// (null_hip.cpp: device memory is host memory, launches compute nothing).  Like the stand-ins there: the first and last element of every
// vector, table and scratch array a launch is handed are touched (a wild or undersized pointer is an ASan report), something plausible is
// written where a kernel would have written its results — every slot's histogram holds all n elements in bin 0, a total the host loop can
// walk (it ends with key 0); the inner sums are 0.25 n; every element lies below the first bound —, the completion flag is raised.
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <cstring>

#include "../../finmath-lib-cuda-extensions_amd/csrc/kernels.h"

namespace fm {

static void os_touch(const DevOsCommon& c, const uint64_t* vecs, uint32_t batch) {
    for (uint32_t k = 0; k < batch; ++k) { const volatile float* p = reinterpret_cast<const float*>((uintptr_t)(c.use_inline ? c.vec0 : vecs[k])); (void)p[0]; (void)p[c.n - 1]; }
    (void)*(volatile uint32_t*)c.counters; (void)((volatile uint32_t*)c.counters)[batch];
}
hipError_t launch_os_hist(const DevSelectArgs& a, const uint64_t* vecs, const uint32_t* slots, uint32_t batch, hipStream_t) {
    os_touch(a.c, vecs, batch);
    for (uint32_t k = 0; k < batch; ++k) {
        const uint32_t* sl = a.c.use_inline ? a.slots0 : slots + (size_t)k * (1u + a.S);
        for (uint32_t s = 0; s < sl[0] && s < a.S; ++s) {
            uint32_t* h = a.hist_host + ((size_t)k * a.S + s) * FM_OS_BINS;
            (void)*(volatile uint32_t*)(a.hist_dev + ((size_t)k * a.S + s) * FM_OS_BINS + FM_OS_BINS - 1);
            std::memset(h, 0, FM_OS_BINS * 4);
            h[0] = (uint32_t)a.c.n;
        }
    }
    __atomic_store_n(a.c.done_flag, a.c.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}
hipError_t launch_os_sum(const DevRankSumArgs& a, const uint64_t* vecs, const uint32_t* keys, uint32_t batch, hipStream_t) {
    os_touch(a.c, vecs, batch);
    const uint32_t blocks = os_sum_blocks(a.c.n);
    for (uint32_t k = 0; k < batch; ++k) {
        if (!a.c.use_inline) (void)*(volatile const uint32_t*)(keys + 2 * (size_t)k + 1);
        a.partials[(size_t)k * blocks] = 0.0; a.partials[(size_t)k * blocks + blocks - 1] = 0.0;
        a.out_host[k] = 0.25 * (double)a.c.n;
    }
    __atomic_store_n(a.c.done_flag, a.c.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}
hipError_t launch_os_count(const DevCountArgs& a, const double* bounds, hipStream_t) {
    os_touch(a.c, nullptr, 1);
    (void)*(volatile const double*)(bounds + a.m - 1); (void)*(volatile uint32_t*)(a.counts_dev + a.m);
    for (uint32_t i = 0; i <= a.m; ++i) a.counts_host[i] = 0u;
    a.counts_host[0] = (uint32_t)a.c.n;
    __atomic_store_n(a.c.done_flag, a.c.done_value, __ATOMIC_RELEASE);
    return hipSuccess;
}

} // namespace fm
