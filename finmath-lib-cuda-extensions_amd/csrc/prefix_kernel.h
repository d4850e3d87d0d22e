// prefix_kernel.h — host-callable launchers of the kernels of prefix_kernel.hip (engine side: prefix_engine.hpp): fp64
// prefix sums of a float vector in the nested tree of prefix_host.hpp — totals per chunk, the carry over the chunks, and the kernel that
// applies it: every prefix as a new vector, or the prefixes at a few positions / at the first crossing of a few thresholds into pinned
// memory.  The constants, the chunk arithmetic and the layout of the scratch are prefix_host.hpp's (no HIP in it:
// tests/cpp/test_prefix_host.cpp drives them on the CPU).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "prefix_host.hpp"

namespace fm {

constexpr uint32_t FM_PREFIX_QUERY_NONE = 0, FM_PREFIX_QUERY_AT = 1, FM_PREFIX_QUERY_SEARCH = 2;

struct DevPrefixArgs {
    uint32_t  n;
    uint32_t  chunk_tiles;     // prefix_chunk_tiles(n); the grid of the totals and the apply kernel is prefix_blocks(n)
    uint32_t  mode;            // FM_PREFIX_SUM / FM_PREFIX_MEAN (launch_prefix_sums)
    uint32_t  kind;            // FM_PREFIX_QUERY_*
    uint32_t  count;           // queries, 1 … FM_PREFIX_MAX_QUERIES (launch_prefix_queries)
    uint32_t  relative;        // thresholds are multiplied by P[n-1]
    uint64_t  v, out;          // addresses of the float vectors, 256-byte aligned and padded
    char*     scratch;         // device: prefix_scratch_bytes(n, count), laid out as prefix_host.hpp says
    double*   total_host;      // pinned; may be null: P[n-1]
    double*   sums_host;       // pinned [count]
    uint64_t* positions_host;  // pinned [count] (search)
};
inline bool prefix_shape_ok(const DevPrefixArgs& a)
{
    return a.n > 0 && a.n <= (uint32_t)FM_PREFIX_MAX_N && a.chunk_tiles == prefix_chunk_tiles(a.n) && a.v && a.scratch && a.mode <= 1u
        && (a.kind == FM_PREFIX_QUERY_NONE ? a.out != 0 && a.out != a.v && a.count == 0u
            : a.kind <= FM_PREFIX_QUERY_SEARCH && a.count >= 1u && a.count <= (uint32_t)FM_PREFIX_MAX_QUERIES && a.sums_host
              && (a.kind == FM_PREFIX_QUERY_AT || a.positions_host));
}
#if defined(__HIP__)
#define FM_PREFIX_HD __host__ __device__
#else
#define FM_PREFIX_HD
#endif
FM_PREFIX_HD inline PrefixRow* prefix_rows(const DevPrefixArgs& a) { return reinterpret_cast<PrefixRow*>(a.scratch); }
FM_PREFIX_HD inline double* prefix_bases(const DevPrefixArgs& a) { return reinterpret_cast<double*>(a.scratch + prefix_rows_bytes(a.n)); }
FM_PREFIX_HD inline uint64_t* prefix_queries(const DevPrefixArgs& a) { return reinterpret_cast<uint64_t*>(a.scratch + prefix_rows_bytes(a.n) + prefix_bases_bytes(a.n)); }
FM_PREFIX_HD inline PrefixLocated* prefix_located(const DevPrefixArgs& a) { return reinterpret_cast<PrefixLocated*>(a.scratch + prefix_rows_bytes(a.n) + prefix_bases_bytes(a.n) + prefix_queries_bytes((int)a.count)); }

// totals → carry → apply (out[r] for every r), chained on `st`
hipError_t launch_prefix_sums(const DevPrefixArgs& a, hipStream_t st);
// totals → carry (which locates every query's chunk) → one workgroup per query, chained on `st`
hipError_t launch_prefix_queries(const DevPrefixArgs& a, hipStream_t st);

} // namespace fm
