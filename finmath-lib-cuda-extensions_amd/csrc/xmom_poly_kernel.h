// xmom_poly_kernel.h — host-callable launchers of fm_xmom_poly_kernel and fm_poly_eval_kernel (xmom_poly_kernel.hip; engine
// side: xmom_poly_engine.hpp; definition: ../host/polynomial_regression.hpp): the normal equations of a regression on a POLYNOMIAL basis of
// up to 8 state vectors, and the fitted polynomial as a new vector, without the monomials ever being in memory.
//
// The moments are fm_xmom_wide_kernel's pass (xmom_wide_kernel.h: the list of 64 slots, the tiles, the tree, the grid, xmom_wide_chain) with
// one more kind of slot: FM_XMOMW_TERM | exponents — a monomial of the state vectors.  A lane loads the four paths of its round of every
// STATE (16 lanes share an address: one request) and forms its own term of every group in registers, by the chain of the contract
// (include/fmhip.h): u^e = ((u·u)·u)…, the powers multiplied in ascending state index, every product rounded to fp32.  The operands of the
// MFMAs are then what the wide kernel would have loaded had the monomials been materialised: the sums are its sums, bit for bit.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "xmom_wide_kernel.h"

namespace fm {

constexpr int FM_POLY_MAX_STATES = 8;
constexpr int FM_POLY_MAX_EXPONENT = 6;
constexpr int FM_POLY_MAX_EVAL = 60;               // terms and extra vectors of one evaluation: the estimator's limit
constexpr int FM_POLY_EVAL_BLOCK = 256;
constexpr int FM_POLY_EVAL_MAX_BLOCKS = 4096;      // the evaluation's grid stops growing here: above 4 · 256 · 4096 elements a lane takes a second quad

// the slot of a term: state s has exponent (slot >> 3s) & 7
inline uint64_t xmom_poly_term_slot(const uint8_t* exponents, int n_states)
{
    uint64_t e = 0;
    for (int s = 0; s < n_states; ++s) e |= (uint64_t)(exponents[s] & 7u) << (3 * s);
    return e ? (FM_XMOMW_TERM | e) : FM_XMOMW_ONE;                 // the all-zero tuple is the constant 1
}

struct DevXmomPolyArgs {
    DevXmomWideArgs w;                             // vec[]: addresses, FM_XMOMW_ONE, FM_XMOMW_PAD or FM_XMOMW_TERM | exponents
    uint64_t state[FM_POLY_MAX_STATES];            // addresses of the state vectors; [n_states, 8) unused
    uint32_t n_states;                             // 1 … 8
    uint32_t max_exponent;                         // the largest exponent of the call, 0 … 6: the bound of the power loop
};
inline bool xmom_poly_shape_ok(const DevXmomPolyArgs& a)
{
    if (!xmom_wide_shape_ok(a.w) || a.n_states < 1 || a.n_states > (uint32_t)FM_POLY_MAX_STATES || a.max_exponent > (uint32_t)FM_POLY_MAX_EXPONENT) return false;
    for (uint32_t s = 0; s < a.n_states; ++s) if (!a.state[s]) return false;
    return true;
}
hipError_t launch_xmom_poly(const DevXmomPolyArgs& a, hipStream_t st);

// r = ((t_0·c_0) + t_1·c_1) + … over the terms, then the extra vectors: one lane per four paths, every product and sum rounded to fp32
struct DevPolyEvalArgs {
    int64_t  n;
    uint64_t out;                                  // storage of n floats, padded to 256 bytes as every vector's is
    uint64_t state[FM_POLY_MAX_STATES];
    uint64_t extra[FM_POLY_MAX_EVAL];              // [n_extra]: an address, or 0 for the constant 1
    uint32_t exponents[FM_POLY_MAX_EVAL];          // [n_terms]: state s at bits 3s … 3s + 2
    float    coefficient[FM_POLY_MAX_EVAL];        // [n_terms + n_extra], narrowed on the host
    uint32_t n_states, n_terms, n_extra;
};
inline bool poly_eval_shape_ok(const DevPolyEvalArgs& a)
{
    if (a.n <= 0 || a.n > (int64_t(1) << 31) || !a.out || a.n_states < 1 || a.n_states > (uint32_t)FM_POLY_MAX_STATES) return false;
    if (a.n_terms < 1 || a.n_terms + a.n_extra > (uint32_t)FM_POLY_MAX_EVAL) return false;
    for (uint32_t s = 0; s < a.n_states; ++s) if (!a.state[s]) return false;
    return true;
}
hipError_t launch_poly_eval(const DevPolyEvalArgs& a, hipStream_t st);

} // namespace fm
