// mt_jump.hpp — jump-ahead for MT19937 (header-only, no HIP): enter the stream of host/mersenne.hpp at any word.
//
// MT19937 is linear over GF(2).  With x[0 … 623] a state and x[624 …] the raw (untempered) words that follow it,
//     x[2^j + k] = XOR over { i : bit i of g_j set } of x[i + k],   k = 0 … 623,   g_j(t) = t^(2^j) mod φ(t),
// φ the minimal polynomial of the recurrence (csrc/fm_mt_jump_table.hpp, written by tools/mt_jump_table.py).  One jump is therefore:
// generate 19936 raw words behind the state, then 624 independent XOR sums — the formulation the device kernel uses too
// (csrc/mt_bm_kernel.hip).  An arbitrary distance is the binary expansion of the distance over the table.
//
// Convention: a state is 624 words of which the low 31 bits of word 0 are NOT part (the recurrence never reads them); after a jump
// they hold no meaning.  The consumer regenerates before it outputs, as MT19937::next32 does with mti = 624, so they never reach an
// output.  jump(state, n) leaves the state from which the next regenerated word is output number n of the stream that `state` starts.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../csrc/fm_mt_jump_table.hpp"
#include "mersenne.hpp"

namespace fmhost {

constexpr uint64_t MT_JUMP_LIMIT = uint64_t(1) << fm::FM_MT_JUMP_COUNT;    // distances 0 … 2^44 − 1 words

// x[624 … count) from x[0 … 624): the raw recurrence, no tempering
inline void mtRawWords(uint32_t* x, size_t count) {
    for (size_t m = 624; m < count; ++m) {
        const uint32_t y = (x[m - 624] & 0x80000000u) | (x[m - 623] & 0x7fffffffu);
        x[m] = x[m - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
}

// state ← the state 2^j words further on
inline void mtJumpPow2(uint32_t* state, int j, std::vector<uint32_t>& raw) {
    constexpr size_t DEGREE = 19937;
    raw.resize(DEGREE + 623);
    for (int k = 0; k < 624; ++k) raw[(size_t)k] = state[k];
    mtRawWords(raw.data(), raw.size());
    uint32_t acc[624] = {};
    const uint32_t* g = fm::FM_MT_JUMP_TABLE[j];
    for (size_t w = 0; w < 624; ++w)
        for (uint32_t bits = g[w]; bits; bits &= bits - 1) {
            const uint32_t* src = raw.data() + 32 * w + (size_t)__builtin_ctz(bits);
            for (int k = 0; k < 624; ++k) acc[k] ^= src[k];
        }
    for (int k = 0; k < 624; ++k) state[k] = acc[k];
}

inline void mtJump(uint32_t* state, uint64_t n_words) {
    if (n_words >= MT_JUMP_LIMIT) throw std::invalid_argument("MT19937 jump-ahead: the distance is limited to 2^44 words");
    std::vector<uint32_t> raw;
    for (int j = 0; n_words; ++j, n_words >>= 1)
        if (n_words & 1u) mtJumpPow2(state, j, raw);
}

// the generator positioned so that its next output is output number n_words of the stream it would have produced from where it stands
inline void mtJump(MT19937& mt, uint64_t n_words) {
    if (mt.mti < 624) {                                 // inside a regenerated block: back to the block's start is not possible, so step to its end
        const uint64_t rest = (uint64_t)(624 - mt.mti);
        if (n_words < rest) { mt.mti += (int)n_words; return; }
        n_words -= rest;                                // words mt[0 … 624) are now the state whose next regenerated word is the next output
    }
    mtJump(mt.mt, n_words);
    mt.mti = 624;
}

} // namespace fmhost
