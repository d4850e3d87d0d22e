// os_device.hpp — the two device functions that every kernel ordering or counting by the 32-bit key of DESIGN.md §4.7 shares: the key itself
// and the wave-peeled LDS count.  Included by kernels.hip (radix select, counting) and sort_kernel.hip (radix sort): one definition of the
// order, not two; binned_kernel.hip counts its bins with os_lds_add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fm {

__device__ __forceinline__ uint32_t os_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    const uint32_t k = (u >> 31) ? ~u : (u | 0x80000000u);
    return ((u & 0x7fffffffu) > 0x7f800000u) ? 0xffffffffu : k;     // NaNs of either sign and any payload: one key, the last
}

// h[bin] += 1 for every lane with `valid`.  Monte-Carlo data is clustered — the leading digit of values in [0.5, 2) is ONE bin, a floored
// payoff is half exact zeros in every pass — and same-address LDS atomics serialise: the most frequent digits of the wave are peeled off
// first, one add of a population count each (at most three rounds, given up as soon as a round finds fewer than eight equal lanes: digits
// that are spread out gain nothing from it); what is left adds lane by lane.
__device__ __forceinline__ void os_lds_add(uint32_t* h, const uint32_t bin, bool valid)
{
    uint64_t pending = __ballot(valid);
#pragma unroll 1
    for (int round = 0; round < 3 && pending != 0ull; ++round) {
        const int leader = __ffsll((long long)pending) - 1;
        const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, leader);
        const uint64_t same = __ballot(valid && bin == b0);
        const uint32_t c = (uint32_t)__popcll(same);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(h + b0, c);
        valid = valid && bin != b0;
        pending &= ~same;
        if (c < 8u) break;
    }
    if (valid) atomicAdd(h + bin, 1u);
}

} // namespace fm
