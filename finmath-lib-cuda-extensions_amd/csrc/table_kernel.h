// table_kernel.h — the host-callable launcher of table_kernel.hip (engine side: table_engine.hpp; definition:
// host/tabulated_function.hpp): up to four tabulated functions on the same knots applied to every element of a vector, one read of the
// vector, one new vector per function.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "../host/tabulated_function.hpp"

namespace fm {

constexpr int FM_TABLE_BLOCK = 256;
constexpr int FM_TABLE_TILE = 1024;                // elements per workgroup and iteration: 256 lanes x 16 bytes
constexpr int FM_TABLE_MAX_BLOCKS = 2048;          // the grid's cap: above FM_TABLE_MAX_BLOCKS * FM_TABLE_TILE elements the grid-stride loop wraps

// The tables of one launch in device memory, as one block that one copy fills: [knots] [coefficients] [first], each part padded to 256 bytes.
inline size_t table_up256(size_t b) { return (b + 255) & ~size_t(255); }
inline size_t table_knots_bytes(int m) { return table_up256((size_t)m * 8); }
inline size_t table_coefficients_bytes(int m, int n_tables) { return table_up256((size_t)n_tables * (size_t)(m + 1) * 32); }
inline size_t table_index_bytes(int cells) { return table_up256((size_t)(cells + 1) * 2); }
inline size_t table_block_bytes(int m, int n_tables, int cells) { return table_knots_bytes(m) + table_coefficients_bytes(m, n_tables) + table_index_bytes(cells); }
// … and in LDS, unpadded: at most 1024·8 + 1028·32 + 2049·2 bytes ≈ 44 KiB
inline size_t table_lds_bytes(int m, int n_tables, int cells) { return (size_t)m * 8 + (size_t)n_tables * (size_t)(m + 1) * 32 + (((size_t)(cells + 1) * 2 + 7) & ~size_t(7)); }

struct DevTableArgs {
    int64_t   n;
    uint32_t  m, n_tables, cells, reserved;
    double    scale;               // of fm_table_cell
    const double*   knots;         // device, [m]
    const double*   coefficients;  // device, [n_tables][m + 1][4]
    const uint16_t* first;         // device, [cells + 1]
    uint64_t  x;                   // addresses (vectors are padded to 256 B)
    uint64_t  out[fmhost::FM_TABLE_MAX_FUNCTIONS];
};
inline uint32_t table_blocks(int64_t n)
{
    const int64_t tiles = (n + FM_TABLE_TILE - 1) / FM_TABLE_TILE;
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_TABLE_MAX_BLOCKS ? FM_TABLE_MAX_BLOCKS : tiles);
}
inline bool table_shape_ok(const DevTableArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31)) return false;
    if (a.m < 1 || a.m > (uint32_t)fmhost::FM_TABLE_MAX_KNOTS || a.n_tables < 1 || a.n_tables > (uint32_t)fmhost::FM_TABLE_MAX_FUNCTIONS) return false;
    if (a.m * a.n_tables > (uint32_t)fmhost::FM_TABLE_MAX_ENTRIES || a.cells != (uint32_t)fmhost::fm_table_cells((int)a.m)) return false;
    if (!(a.scale >= 0.0) || a.scale - a.scale != 0.0) return false;
    if (!a.knots || !a.coefficients || !a.first || !a.x) return false;
    for (uint32_t f = 0; f < a.n_tables; ++f) if (!a.out[f]) return false;
    return true;
}
hipError_t launch_table_apply(const DevTableArgs& a, hipStream_t st);

} // namespace fm
