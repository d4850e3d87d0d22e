#!/usr/bin/env python3
"""Direction numbers of the Sobol' sequence: host/sobol_directions.hpp.

The table is Joe & Kuo's `new-joe-kuo-6`, first 1024 dimensions, in its compact form: per dimension the degree s of the primitive
polynomial, its inner coefficients a (a_1 … a_(s-1) as the bits of one integer, a_1 the most significant) and the initial numbers
m_1 … m_s.  host/sobol.hpp expands it to 30-bit direction words by the standard recurrence

    v_j = m_j · 2^(30 - j)                                                              j = 1 … s
    v_j = v_(j-s) ^ (v_(j-s) >> s) ^ a_1 v_(j-1) ^ … ^ a_(s-1) v_(j-s+1)                j = s + 1 … 30

(dimension 1: v_j = 2^(30 - j)).  Nothing is downloaded: the expanded words of exactly this table ship with PyTorch
(torch.quasirandom.SobolEngine(1024, scramble=False).sobolstate, [1024, 30]), and the compact form is recovered from them — m_j is the
top j bits of v_j; s and a are the smallest degree and the one candidate among 2^(s-1) whose recurrence reproduces every later word.
The degrees found must be the primitive-polynomial counts of the table's ordering (1, 1, 2, 2, 6, 6, 18, 16, 48, 60, 176, 144, 630 …).

    python tools/sobol_directions.py            # (re)write the header
    python tools/sobol_directions.py --check    # recompute, compare with the committed header, exit 1 on drift
"""
import os
import sys

DIMS, BITS, MAX_DEGREE = 1024, 30, 13
PRIMITIVE_POLYNOMIALS = [1, 1, 2, 2, 6, 6, 18, 16, 48, 60, 176, 144, 630]        # per degree 1 … 13, over GF(2)
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "finmath-lib-cuda-extensions_amd", "host", "sobol_directions.hpp")

NOTICE = """\
// The numbers below are the direction numbers `new-joe-kuo-6` of
//   S. Joe and F. Y. Kuo, Constructing Sobol sequences with better two-dimensional projections, SIAM J. Sci. Comput. 30, 2635-2654 (2008),
// first 1024 dimensions, distributed by their authors under this licence:
//
//   Copyright (c) 2008, Frances Y. Kuo and Stephen Joe.  All rights reserved.
//
//   Redistribution and use in source and binary forms, with or without modification, are permitted provided that the following
//   conditions are met:
//     * Redistributions of source code must retain the above copyright notice, this list of conditions and the following disclaimer.
//     * Redistributions in binary form must reproduce the above copyright notice, this list of conditions and the following
//       disclaimer in the documentation and/or other materials provided with the distribution.
//     * Neither the names of the copyright holders nor the names of the University of New South Wales and the University of Waikato
//       and its contributors may be used to endorse or promote products derived from this software without specific prior written
//       permission.
//
//   THIS SOFTWARE IS PROVIDED BY THE COPYRIGHT HOLDERS ``AS IS'' AND ANY EXPRESS OR IMPLIED WARRANTIES, INCLUDING, BUT NOT LIMITED
//   TO, THE IMPLIED WARRANTIES OF MERCHANTABILITY AND FITNESS FOR A PARTICULAR PURPOSE ARE DISCLAIMED.  IN NO EVENT SHALL THE
//   COPYRIGHT HOLDERS BE LIABLE FOR ANY DIRECT, INDIRECT, INCIDENTAL, SPECIAL, EXEMPLARY, OR CONSEQUENTIAL DAMAGES (INCLUDING, BUT
//   NOT LIMITED TO, PROCUREMENT OF SUBSTITUTE GOODS OR SERVICES; LOSS OF USE, DATA, OR PROFITS; OR BUSINESS INTERRUPTION) HOWEVER
//   CAUSED AND ON ANY THEORY OF LIABILITY, WHETHER IN CONTRACT, STRICT LIABILITY, OR TORT (INCLUDING NEGLIGENCE OR OTHERWISE)
//   ARISING IN ANY WAY OUT OF THE USE OF THIS SOFTWARE, EVEN IF ADVISED OF THE POSSIBILITY OF SUCH DAMAGE.
"""


def expand(s, a, m):
    """The 30 direction words of one dimension from its compact form (s = 0: the first dimension)."""
    if s == 0:
        return [1 << (BITS - 1 - j) for j in range(BITS)]
    v = [m[j] << (BITS - 1 - j) for j in range(min(s, BITS))]
    for j in range(s, BITS):
        w = v[j - s] ^ (v[j - s] >> s)
        for k in range(1, s):
            if (a >> (s - 1 - k)) & 1:
                w ^= v[j - k]
        v.append(w)
    return v


def compact(words):
    """(s, a, m) of one dimension's 30 words: the smallest degree with a coefficient set that reproduces them."""
    for s in range(1, MAX_DEGREE + 1):
        m = [words[j] >> (BITS - 1 - j) for j in range(s)]
        if any(words[j] != m[j] << (BITS - 1 - j) or not m[j] & 1 for j in range(s)):
            continue
        for a in range(1 << (s - 1)):
            taps = [k for k in range(1, s) if (a >> (s - 1 - k)) & 1]
            for j in range(s, BITS):                      # most candidates fail at the first word
                w = words[j - s] ^ (words[j - s] >> s)
                for k in taps:
                    w ^= words[j - k]
                if w != words[j]:
                    break
            else:
                assert expand(s, a, m) == words
                return s, a, m
    raise SystemExit("no recurrence of degree <= 13 reproduces a dimension's direction words")


def table():
    import torch
    state = torch.quasirandom.SobolEngine(dimension=DIMS, scramble=False).sobolstate
    if tuple(state.shape) != (DIMS, BITS):
        raise SystemExit(f"sobolstate has shape {tuple(state.shape)}, expected {(DIMS, BITS)}")
    rows = [[int(x) for x in row] for row in state.tolist()]
    if rows[0] != expand(0, 0, []):
        raise SystemExit("the first dimension is not the van der Corput sequence")
    out = [(0, 0, [])] + [compact(r) for r in rows[1:]]
    degrees = [s for s, _, _ in out[1:]]
    want = [d + 1 for d, count in enumerate(PRIMITIVE_POLYNOMIALS) for _ in range(count)][:DIMS - 1]
    if degrees != want:
        raise SystemExit("the degrees found are not those of the table's ordering")
    return out


def render(rows):
    lines = ["// sobol_directions.hpp: GENERATED by tools/sobol_directions.py; do not edit.  Read by host/sobol.hpp alone.",
             "//", NOTICE.rstrip("\n"), "//",
             "// Per dimension: degree s, coefficients a (a_1 … a_(s-1), a_1 the most significant bit), then m_1 … m_s; FM_SOBOL_ROW_START[d] is the",
             "// index of dimension d's s in FM_SOBOL_COMPACT.  Dimension 0 has s = 0: v_j = 2^(30 - j).",
             "#pragma once", "#include <stdint.h>", "", "namespace fmhost {", "",
             f"constexpr int FM_SOBOL_DIMS = {DIMS}, FM_SOBOL_BITS = {BITS};", ""]
    flat, starts = [], []
    for s, a, m in rows:
        starts.append(len(flat))
        flat += [s, a] + m
    lines.append(f"static const uint16_t FM_SOBOL_COMPACT[{len(flat)}] = {{")
    for s, a, m in rows:
        lines.append("    " + ",".join(str(x) for x in [s, a] + m) + ",")
    lines.append("};")
    lines.append("")
    lines.append(f"static const uint16_t FM_SOBOL_ROW_START[{DIMS}] = {{")
    for k in range(0, DIMS, 32):
        lines.append("    " + ",".join(str(x) for x in starts[k:k + 32]) + ",")
    lines.append("};")
    lines += ["", "} // namespace fmhost", ""]
    assert max(flat) < 65536 and max(starts) < 65536
    return "\n".join(lines)


def main():
    text = render(table())
    if "--check" in sys.argv[1:]:
        with open(HEADER) as fh:
            if fh.read() != text:
                print("host/sobol_directions.hpp differs from what the tool generates", file=sys.stderr)
                return 1
        print("host/sobol_directions.hpp is current")
        return 0
    with open(HEADER, "w") as fh:
        fh.write(text)
    print(f"wrote {os.path.normpath(HEADER)} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
