// xmom_wide_kernel.h — host-callable launcher of fm_xmom_wide_kernel (xmom_wide_kernel.hip; engine side:
// xmom_wide_engine.hpp): S[i][j] = Σ_p x_i[p]·x_j[p] and T[i][m] = Σ_p x_i[p]·y_m[p] in fp64 for up to 64 vectors of one size in ONE launch, on
// the matrix cores (v_mfma_f64_16x16x4_f64).
//
// The vectors form one list (x then y), cut into groups of 16; a short group is padded with zero operands, which are not loaded.  A wave
// keeps one 16 x 16 accumulator tile per pair of groups (g, h), g <= h: tile g·(7 - g)/2 + h, ten tiles for four groups.  A workgroup reads
// every vector of the call once.
//
// Order of the additions of ONE pair (the tree; it is a function of n alone — not of the number of vectors, of the group or the row a
// vector falls into, of which of the two is the A operand, or of the roles):
//   - paths are cut into CHUNKS of 64 (the 256 bytes a vector is padded to); chunk c belongs to wave (c mod W) of the launch, W = 8 x grid,
//     wave w of workgroup b being number b·8 + w; a wave adds its chunks in ascending order, each chunk by 16 MFMAs in a fixed order, each
//     MFMA adding the exact products of 4 paths to the running sum (paths past n contribute +0.0·+0.0);
//   - the 8 waves of a workgroup are added in order, ((w0 + w1) + w2) + …;
//   - the workgroups' partials are added in order, ((b0 + b1) + b2) + …, by the last workgroup to arrive.
// Longest chain of additions: xmom_wide_chain(n) below.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace fm {

constexpr int FM_XMOMW_MAX = 64;                   // vectors of one call, x and y together
constexpr int FM_XMOMW_GROUP = 16;                 // the MFMA's tile edge
constexpr int FM_XMOMW_MAX_GROUPS = FM_XMOMW_MAX / FM_XMOMW_GROUP;
constexpr int FM_XMOMW_MAX_TILES = FM_XMOMW_MAX_GROUPS * (FM_XMOMW_MAX_GROUPS + 1) / 2;       // 10
constexpr int FM_XMOMW_TILE_ENTRIES = FM_XMOMW_GROUP * FM_XMOMW_GROUP;
constexpr int FM_XMOMW_BLOCK = 512;                // 8 waves: two per SIMD
constexpr int FM_XMOMW_WAVES = FM_XMOMW_BLOCK / 64;
constexpr int FM_XMOMW_CHUNK = 64;                 // paths a wave takes at a time: 256 bytes of every vector
constexpr int FM_XMOMW_TILE = FM_XMOMW_WAVES * FM_XMOMW_CHUNK;     // paths per workgroup and iteration: 512
constexpr int FM_XMOMW_MAX_GRID = 256;             // one workgroup per CU

// what a slot of the list holds instead of an address (no vector lives at either)
constexpr uint64_t FM_XMOMW_PAD = 0, FM_XMOMW_ONE = 1;
// … and, for fm_xmom_poly_kernel only (xmom_poly_kernel.h), a monomial the lane forms itself: this tag (no address has bit 63) beside the
// exponents of up to 8 state vectors, 3 bits each, state s at bits 3s … 3s + 2
constexpr uint64_t FM_XMOMW_TERM = uint64_t(1) << 63;

struct DevXmomWideArgs {
    uint32_t* counter;         // one arrival counter; zero before and after
    uint64_t* done_flag;       // pinned; receives done_value when out_host is in host memory
    uint64_t  done_value;
    int64_t   n;
    uint32_t  chunks;          // ceil(n / FM_XMOMW_CHUNK)
    uint32_t  n_groups;        // 1 … 4
    uint64_t  vec[FM_XMOMW_MAX];                   // addresses, by value as fm_xmom_kernel's; FM_XMOMW_ONE = the constant 1, FM_XMOMW_PAD = a zero operand
    double*   partials;        // device [grid][FM_XMOMW_MAX_TILES][256]; the tiles of n_groups groups are written
    double*   out_host;        // pinned [FM_XMOMW_MAX_TILES][256]: see xmom_wide_entry
};

constexpr uint32_t xmom_wide_tiles(uint32_t n_groups) { return n_groups * (n_groups + 1u) / 2u; }
// workgroups: a function of n ONLY — the order of the fp64 additions depends on nothing else.  Two chunks per wave before the grid grows:
// the last workgroup adds grid x tiles x 256 partials, which is what a small call pays for.
inline uint32_t xmom_wide_blocks(int64_t n)
{
    const int64_t tiles = (n + 2 * FM_XMOMW_TILE - 1) / (2 * FM_XMOMW_TILE);
    return (uint32_t)(tiles < 1 ? 1 : tiles > FM_XMOMW_MAX_GRID ? FM_XMOMW_MAX_GRID : tiles);
}
// L(n): the longest chain of additions behind one sum — 64 per chunk of a wave (16 MFMAs of 4 paths), 7 for the waves, grid - 1 for the
// workgroups.  |computed - exact| <= (L(n) + 1)·2^-53·Σ|a·b| to first order.
inline int64_t xmom_wide_chain(int64_t n)
{
    const int64_t grid = xmom_wide_blocks(n), waves = grid * FM_XMOMW_WAVES;
    const int64_t chunks = (n + FM_XMOMW_CHUNK - 1) / FM_XMOMW_CHUNK;
    return FM_XMOMW_CHUNK * ((chunks + waves - 1) / waves) + (FM_XMOMW_WAVES - 1) + (grid - 1);
}
// where Σ list[i]·list[j] (i <= j) stands in out_host: tile (g, h) of the groups, A operand = group g; the f64 MFMA's result map is
// col = lane & 15, row = (lane >> 4) + 4·reg (NOT the f32 forms' map), stored as [reg][lane]
inline size_t xmom_wide_entry(int i, int j)
{
    const int g = i / FM_XMOMW_GROUP, h = j / FM_XMOMW_GROUP, row = i % FM_XMOMW_GROUP, col = j % FM_XMOMW_GROUP;
    const int tile = g * (2 * FM_XMOMW_MAX_GROUPS - 1 - g) / 2 + h;
    return (size_t)tile * FM_XMOMW_TILE_ENTRIES + (size_t)(row >> 2) * 64 + (size_t)(col + 16 * (row & 3));
}
inline bool xmom_wide_shape_ok(const DevXmomWideArgs& a)
{
    return a.n > 0 && a.n <= (int64_t(1) << 31) && a.chunks == (uint32_t)((a.n + FM_XMOMW_CHUNK - 1) / FM_XMOMW_CHUNK)
        && a.n_groups >= 1 && a.n_groups <= (uint32_t)FM_XMOMW_MAX_GROUPS && a.counter && a.done_flag && a.partials && a.out_host;
}
hipError_t launch_xmom_wide(const DevXmomWideArgs& a, hipStream_t st);

} // namespace fm
