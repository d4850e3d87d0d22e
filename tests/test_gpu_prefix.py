"""Prefix sums on the device (include/fmhip.h: fmhip_prefix_sums, fmhip_prefix_sums_at, fmhip_prefix_search) through the
C-ABI and the Python mirror.  The tree is the contract, so every check is an EQUALITY: with the host definition (fmhip_prefix_sums_host,
itself checked against math.fsum and numpy in tests/test_prefix_cpu.py) or with numpy on data whose sums are exact.  Of a NaN only that it
is one.  Sizes come from the constants of csrc/prefix_host.hpp, read from the header, and every size asserts the regime it is there for.
No test here asks the device for anything out of range: bad arguments are refused on the host before a launch, and the largest n is a
few million.  Sizes near 2^31 - 1 are covered by the arithmetic checks of tests/cpp/test_prefix_host.cpp alone."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_prefix_cpu import ITEMS, K, TILE, WAVE, blocks, chunk_tiles, definition, dyadic, inputs, same_f64, wide_range
from test_sort_cpu import keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNK = chunk_tiles(1) * TILE                   # one workgroup's chunk while the table of rows is not full
THREE = 2 * CHUNK + 1                           # the smallest n with three workgroups …
while THREE % TILE == 0 or THREE % 64 == 0: THREE += 1      # … (it is) and a ragged tail
FULL = K["FM_PREFIX_MAX_BLOCKS"] * CHUNK        # the largest n of minimal chunks
PAST = FULL + TILE + 3                          # just past a full table of rows: chunks exceed the minimum
assert CHUNK >= 2 * TILE                        # the tile-to-tile carry runs at test sizes
assert blocks(THREE) == 3 and blocks(THREE - 1) == 2 and blocks(CHUNK) == 1 and blocks(CHUNK + 1) == 2
assert chunk_tiles(FULL) == chunk_tiles(1) and blocks(FULL) == K["FM_PREFIX_MAX_BLOCKS"] and chunk_tiles(PAST) == chunk_tiles(1) + 1 and PAST < 6_000_000
SIZES = sorted({1, 2, ITEMS - 1, ITEMS, ITEMS + 1, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, THREE, 100_003})
MAXQ = K["FM_PREFIX_MAX_QUERIES"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_f32(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def rounded(p, mean):
    with np.errstate(over="ignore", invalid="ignore"):
        return (p / np.arange(1, p.size + 1, dtype=np.float64) if mean else p).astype(np.float32)


def first_crossing(p, t):
    """(position, sum) of the definition of fmhip_prefix_search over the definition's prefixes."""
    with np.errstate(invalid="ignore"):
        hit = p >= t
    r = int(np.argmax(hit)) if hit.any() else p.size
    return r, (p[r] if r < p.size else p[-1])


def boundary_positions(n):
    c = chunk_tiles(n) * TILE
    return sorted({r for r in (0, 1, ITEMS - 1, ITEMS, 63, 64, WAVE - 1, WAVE, TILE - 1, TILE, TILE + 1, c - 1, c, c + 1, 2 * c - 1, 2 * c, n // 2, n - 2, n - 1) if 0 <= r < n})


@pytest.mark.parametrize("n", SIZES)
def test_both_modes_are_the_definition_rounded(gpu, n):
    rng = np.random.default_rng(n)
    for name, a in inputs(n, rng):
        v = gpu.DeviceVector.from_host(a)
        p = definition(gpu, a)
        out, total = gpu.cumulative_sums(v, with_total=True)
        assert same_f32(out.to_float32(), rounded(p, False)), (name, n)
        assert same_f64(total, p[-1]), (name, n)
        assert same_f32(gpu.running_average(v).to_float32(), rounded(p, True)), (name, n)
        assert (bits(v.to_float32()) == bits(a)).all(), (name, n)              # the input is unchanged
        if name == "signed zeros" and a[0] == 0 and np.signbit(a[0]):
            lead = int(np.argmin(np.signbit(a))) if not np.signbit(a).all() else n
            assert np.signbit(out.to_float32()[:lead]).all()                    # a leading -0.0 stays -0.0


def test_a_size_just_past_a_full_table_of_rows(gpu):
    """Chunks of three tiles, 1024 rows but for the ragged last: both modes, the prefixes at every kind of boundary, first crossings."""
    n = PAST
    rng = np.random.default_rng(17)
    for name, a in (("wide range", wide_range(n, rng)), ("wide range, signed", wide_range(n, rng, signed=True)), ("dyadic", dyadic(n, rng))):
        v = gpu.DeviceVector.from_host(a)
        p = definition(gpu, a)
        out, total = gpu.cumulative_sums(v, with_total=True)
        assert same_f32(out.to_float32(), rounded(p, False)) and same_f64(total, p[-1]), name
        assert same_f32(gpu.running_average(v).to_float32(), rounded(p, True)), name
        pos = boundary_positions(n)
        assert same_f64(gpu.prefix_sums_at(v, pos), p[pos]), name
        ts = np.concatenate([p[pos], np.nextafter(p[pos], -np.inf), np.nextafter(p[pos], np.inf)])
        where, sums, tot = gpu.prefix_search(v, ts)
        want = [first_crossing(p, t) for t in ts]
        assert (where == [w[0] for w in want]).all() and same_f64(sums, [w[1] for w in want]) and same_f64(tot, p[-1]), name
        if name != "wide range, signed": assert (np.diff(out.to_float32()) >= 0).all()


@pytest.mark.parametrize("n", [1, ITEMS + 1, 65, TILE + 1, CHUNK, THREE, 100_003])
def test_prefix_sums_at_boundaries_repeats_and_4096_positions(gpu, n):
    rng = np.random.default_rng(n + 5)
    for name, a in (("wide range, signed", wide_range(n, rng, signed=True)), ("dyadic", dyadic(n, rng))):
        v = gpu.DeviceVector.from_host(a)
        p = definition(gpu, a)
        pos = boundary_positions(n)
        pos = pos + pos[::-1] + [pos[0]] * 3                                    # any order, repeats
        assert same_f64(gpu.prefix_sums_at(v, pos), p[pos]), (name, n)
        many = rng.integers(0, n, MAXQ)
        got = gpu.prefix_sums_at(v, many)
        assert same_f64(got, p[many]), (name, n)
        # consistency: rounded to fp32, these are the output vector's elements
        assert same_f32(got.astype(np.float32), gpu.cumulative_sums(v).to_float32()[many]), (name, n)
        assert same_f64(gpu.prefix_sums_at(v, [n - 1]), p[-1:])


@pytest.mark.parametrize("n", [1, 65, TILE + 1, THREE, 100_003])
def test_search_finds_the_first_crossing(gpu, n):
    rng = np.random.default_rng(n + 9)
    for name, a in (("dyadic", dyadic(n, rng)), ("wide range", wide_range(n, rng)), ("wide range, signed", wide_range(n, rng, signed=True)), ("normal", rng.standard_normal(n).astype(np.float32))):
        v = gpu.DeviceVector.from_host(a)
        p = definition(gpu, a)
        at = np.array(boundary_positions(n) + rng.integers(0, n, 200).tolist())
        ts = np.concatenate([p[at], np.nextafter(p[at], -np.inf), np.nextafter(p[at], np.inf),                 # a prefix exactly, just below, just above
                             [p[0], np.nextafter(p[0], -np.inf), -np.inf, p.min(), p.max(), np.nextafter(p.max(), np.inf), np.inf, np.nan, 0.0]])
        where, sums, total = gpu.prefix_search(v, ts)
        want = [first_crossing(p, t) for t in ts]
        assert where.dtype == np.int64 and (where == [w[0] for w in want]).all(), (name, n)
        assert same_f64(sums, [w[1] for w in want]) and same_f64(total, p[-1]), (name, n)
        assert where[-2] == n and where[-3] == n and sums[-2] == p[-1]          # a NaN threshold and +inf find nothing: n and P[n-1]
        if name == "dyadic":
            # an exact hit is a hit: on dyadic data the thresholds that equal a prefix find the first position with that prefix
            exact, _, _ = gpu.prefix_search(v, p[at][:MAXQ])
            assert (exact == np.searchsorted(p, p[at], side="left")).all()


def test_relative_thresholds_with_trailing_zero_weights(gpu):
    n = THREE
    w = dyadic(n, np.random.default_rng(3)); w[0] = 0.0; w[n - 700:] = 0.0
    v = gpu.DeviceVector.from_host(w)
    p = np.cumsum(w, dtype=np.float64)                                          # exact
    levels = np.array([0.0, 0.5, 1.0, 0.25, 1.0 + 2.0 ** -40, np.nan])
    where, sums, total = gpu.prefix_search(v, levels, relative=True)
    assert total == p[-1]
    want = [first_crossing(p, t) for t in levels * p[-1]]
    assert (where == [x[0] for x in want]).all() and same_f64(sums, [x[1] for x in want])
    assert where[0] == 0 and where[2] == int(np.flatnonzero(w)[-1]) and where[2] < n - 700 and where[4] == n and where[5] == n      # level 1: the last positive weight, not the last path


def test_signed_input_whose_first_crossing_is_in_an_earlier_chunk(gpu):
    """The running sum climbs to 10 inside the first chunk and is back at 0 at its end; the second chunk climbs to 20.  The first crossing
    of 5 is in the FIRST chunk, whose total does not reach it: the chunks are found by their largest prefix, not by their totals."""
    n = 3 * CHUNK
    a = np.zeros(n, dtype=np.float32)
    a[100:110] = 1.0; a[CHUNK - 20:CHUNK - 10] = -1.0
    a[CHUNK + 50:CHUNK + 70] = 1.0
    a[2 * CHUNK + 5] = -30.0
    p = np.cumsum(a, dtype=np.float64)
    assert p[CHUNK - 1] == 0 and p[:CHUNK].max() == 10 and p[2 * CHUNK - 1] == 20 and p[-1] == -10
    v = gpu.DeviceVector.from_host(a)
    ts = np.array([5.0, 10.0, 10.5, 20.0, 20.5, -5.0, -10.0, 0.0, 1.0])
    where, sums, total = gpu.prefix_search(v, ts)
    want = [first_crossing(p, t) for t in ts]
    assert (where == [x[0] for x in want]).all() and same_f64(sums, [x[1] for x in want]) and total == -10
    assert where[0] == 104 and where[2] == CHUNK + 60 and where[4] == n and where[5] == 0
    # relative to a negative total: level 1 is the first prefix >= -10, level -1 the first >= 10
    where, _, _ = gpu.prefix_search(v, [1.0, -1.0, -2.0, -2.5], relative=True)
    assert where.tolist() == [0, 109, CHUNK + 69, n]


def test_nan_and_infinity_propagate_and_never_qualify(gpu):
    n = THREE
    base = np.random.default_rng(8).random(n, dtype=np.float32)
    for at in (0, ITEMS, 64, WAVE - 1, TILE, CHUNK - 1, CHUNK, 2 * CHUNK, n - 1):
        a = base.copy(); a[at] = np.nan
        v = gpu.DeviceVector.from_host(a)
        p = definition(gpu, a)
        out, total = gpu.cumulative_sums(v, with_total=True)
        got = out.to_float32()
        assert (np.isnan(got) == (np.arange(n) >= at)).all() and same_f32(got, rounded(p, False)) and math.isnan(total), at
        where, sums, _ = gpu.prefix_search(v, [0.0, p[max(at - 1, 0)], 1e30, -np.inf])
        want = [first_crossing(p, t) for t in (0.0, p[max(at - 1, 0)], 1e30, -np.inf)]
        assert (where == [x[0] for x in want]).all() and same_f64(sums, [x[1] for x in want]), at
        if at + 1 < n:
            a[at] = np.inf; a[at + 1] = -np.inf
            v = gpu.DeviceVector.from_host(a)
            p = definition(gpu, a)
            got = gpu.cumulative_sums(v).to_float32()
            assert same_f32(got, rounded(p, False)) and got[at] == np.inf and np.isnan(got[at + 1:]).all(), at
            where, sums, _ = gpu.prefix_search(v, [1e30, np.inf])
            assert where.tolist() == [at, at] and (sums == np.inf).all()


# ---------------------------------------------------------------- weighted statistics
def weighted_reference(x, w, levels):
    order = np.argsort(keys(x), kind="stable")
    sx, sw = x[order], w[order]
    cw = np.cumsum(sw, dtype=np.float64)                                        # exact on dyadic weights
    pos = [first_crossing(cw, level * cw[-1])[0] for level in levels]
    return sx, sw, cw, pos


@pytest.mark.parametrize("n", [1, 65, THREE, 100_003])
def test_weighted_quantiles_and_expected_shortfall_on_dyadic_weights(gpu, n):
    rng = np.random.default_rng(n + 21)
    x = rng.integers(-50, 51, n).astype(np.float32)                             # ties: in path order
    w = dyadic(n, rng)
    if n > 1: w[rng.integers(0, n, n // 10 + 1)] = 0.0
    if w.sum() == 0: w[0] = 2.0 ** -20
    levels = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]
    sx, sw, cw, pos = weighted_reference(x, w, levels)
    X, W = gpu.DeviceVector.from_host(x), gpu.DeviceVector.from_host(w)
    got = gpu.weighted_quantiles(X, W, levels)
    assert same_f64(got, sx[pos].astype(np.float64))
    wx = np.cumsum((sw * sx).astype(np.float64), dtype=np.float64)              # the fp32 products are exact (|k·x| < 2^18), and so are their sums
    for level, r in zip(levels, pos):
        if cw[r] == 0: continue                                                 # (no weight up to there: 0 / 0)
        assert same_f64(gpu.weighted_expected_shortfall(X, W, level), wx[r] / cw[r]), level
    assert math.isnan(gpu.weighted_quantiles(X, W, [1.5])[0]) and math.isnan(gpu.weighted_quantiles(X, W, [np.nan])[0])


@pytest.mark.parametrize("n", [1, 64, THREE, 100_003])
def test_with_equal_weights_the_weighted_quantile_is_the_sorted_element(gpu, n):
    rng = np.random.default_rng(n + 22)
    x = rng.standard_normal(n).astype(np.float32)
    levels = np.array([0.001, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0])
    got = gpu.weighted_quantiles(gpu.DeviceVector.from_host(x), gpu.DeviceVector.filled(n, 1.0), levels)
    ranks = np.maximum(np.ceil(levels * n).astype(np.int64) - 1, 0)
    assert same_f64(got, np.sort(x)[ranks].astype(np.float64))


@pytest.mark.parametrize("n", [1, 65, THREE, 100_003])
def test_expected_shortfall_curve_on_integer_valued_losses(gpu, n):
    x = np.random.default_rng(n + 23).integers(-1000, 1001, n).astype(np.float32)
    want = (np.cumsum(np.sort(x), dtype=np.float64) / np.arange(1, n + 1)).astype(np.float32)
    assert (bits(gpu.expected_shortfall_curve(gpu.DeviceVector.from_host(x)).to_float32()) == bits(want)).all()
    rv = gpu.RandomVariableHipFactory().createRandomVariable(0.0, x.astype(np.float64))
    assert (bits(gpu.expected_shortfall_curve(rv).to_float32()) == bits(want)).all()


# ---------------------------------------------------------------- the engine's behaviour
def test_pending_operands_give_the_bits_of_materialised_ones(gpu):
    n = THREE
    a = wide_range(n, np.random.default_rng(3), signed=True)
    prev = gpu.set_fusion(True)
    try:
        stored = gpu.DeviceVector.from_host(a)
        doubled = gpu.DeviceVector.from_host((a * np.float32(2.0)).astype(np.float32))
        pos, ts = boundary_positions(n), [0.0, 0.5, 1.0]
        want = [gpu.cumulative_sums(doubled).to_float32(), gpu.running_average(doubled).to_float32(), gpu.prefix_sums_at(doubled, pos), gpu.prefix_search(doubled, ts, relative=True)]
        got = [gpu.cumulative_sums(stored.v1s1("MULT_S", 2.0)).to_float32(), gpu.running_average(stored.v1s1("MULT_S", 2.0)).to_float32(),
               gpu.prefix_sums_at(stored.v1s1("MULT_S", 2.0), pos), gpu.prefix_search(stored.v1s1("MULT_S", 2.0), ts, relative=True)]
        assert same_f32(got[0], want[0]) and same_f32(got[1], want[1]) and same_f64(got[2], want[2])
        assert (got[3][0] == want[3][0]).all() and same_f64(got[3][1], want[3][1]) and same_f64(got[3][2], want[3][2])
        assert (bits(stored.to_float32()) == bits(a)).all()
    finally:
        gpu.set_fusion(prev)


def test_pool_statistics_show_only_the_outputs(gpu):
    n = 100_003
    a = np.random.default_rng(8).random(n, dtype=np.float32)
    v = gpu.DeviceVector.from_host(a)
    gpu.cumulative_sums(v); gpu.prefix_sums_at(v, [0]); gpu.prefix_search(v, [0.5])       # warm: scratch and pinned blocks are the engine's for good
    before = gpu.pool_stats().bytes_in_use
    probe = gpu.DeviceVector.from_host(a)
    per_vector = gpu.pool_stats().bytes_in_use - before
    del probe
    assert per_vector >= 4 * n
    for call, n_out in ((lambda: gpu.cumulative_sums(v), 1), (lambda: gpu.running_average(v), 1), (lambda: gpu.prefix_sums_at(v, [0, n - 1]), 0), (lambda: gpu.prefix_search(v, [0.5], relative=True), 0)):
        before = gpu.pool_stats()
        kept = call()
        after = gpu.pool_stats()
        assert after.n_live_vectors - before.n_live_vectors == n_out
        assert after.bytes_in_use - before.bytes_in_use == n_out * per_vector
        assert after.n_kernel_launches == before.n_kernel_launches + 1          # ONE armed launch per call
        del kept


def test_refusals_are_made_on_the_host(gpu):
    N = gpu._native
    lib = gpu.lib()
    n = 1000
    v = gpu.DeviceVector.from_host(np.arange(n, dtype=np.float32))
    before = gpu.pool_stats()
    h, total = C.c_int64(0), C.c_double(-1.0)
    sums, where = (C.c_double * 3)(), (C.c_int64 * 3)()
    i64, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    assert lib.fmhip_prefix_sums(v.handle, 2, C.byref(h), C.byref(total)) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums(v.handle, -1, C.byref(h), None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums(v.handle, 0, None, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums(0, 0, C.byref(h), None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums(v.handle + 12345, 0, C.byref(h), None) == N.ERR_INVALID_HANDLE
    for bad in ([-1], [n], [0, 5, n], [1 << 40]):
        p = np.array(bad, dtype=np.int64)
        assert lib.fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(i64), p.size, sums) == N.ERR_INVALID_ARGUMENT, bad
    p = np.zeros(MAXQ + 1, dtype=np.int64); t = np.zeros(MAXQ + 1, dtype=np.float64); big = np.zeros(MAXQ + 1, dtype=np.float64)
    assert lib.fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(i64), 0, sums) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(i64), MAXQ + 1, big.ctypes.data_as(f64)) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums_at(v.handle, None, 1, sums) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(i64), 1, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_search(v.handle, t.ctypes.data_as(f64), 0, 0, where, sums, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_search(v.handle, t.ctypes.data_as(f64), MAXQ + 1, 0, p.ctypes.data_as(i64), big.ctypes.data_as(f64), None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_search(v.handle, None, 1, 0, where, sums, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_search(v.handle, t.ctypes.data_as(f64), 1, 0, None, sums, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_prefix_search(v.handle, t.ctypes.data_as(f64), 1, 0, where, None, None) == N.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gpu.prefix_sums_at(v, [n])
    with pytest.raises(ValueError):
        gpu.prefix_search(v, np.zeros(MAXQ + 1))
    # a communicator of two ranks: a carry between the ranks is not built
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        assert lib.fmhip_prefix_sums(v.handle, 0, C.byref(h), C.byref(total)) == N.ERR_UNSUPPORTED
        assert lib.fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(i64), 1, sums) == N.ERR_UNSUPPORTED
        assert lib.fmhip_prefix_search(v.handle, t.ctypes.data_as(f64), 1, 1, where, sums, C.byref(total)) == N.ERR_UNSUPPORTED
    finally:
        gpu.set_expectation_comm(1, 0, None)
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors      # nothing was launched for any of it
    assert h.value == 0 and total.value == -1.0
    assert gpu.prefix_sums_at(v, [n - 1])[0] == n * (n - 1) / 2


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
        ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 4)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for y in ys:
            try:
                y.to_float32()
                read_error = None
            except gpu.FmhipError as e:
                read_error = e.code
            for call in (lambda: gpu.cumulative_sums(y), lambda: gpu.prefix_sums_at(y, [0]), lambda: gpu.prefix_search(y, [1.0])):
                if read_error is None:
                    call()
                else:
                    with pytest.raises(gpu.FmhipError) as info:
                        call()
                    assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


def test_the_host_switch_gives_identical_results(gpu, monkeypatch):
    n = THREE
    rng = np.random.default_rng(6)
    a, x = wide_range(n, rng, signed=True), rng.integers(-50, 51, n).astype(np.float32)
    w = dyadic(n, rng)
    pos, levels = boundary_positions(n), [0.0, 0.1, 0.5, 0.9, 1.0]
    def everything():
        v, X, W = gpu.DeviceVector.from_host(a), gpu.DeviceVector.from_host(x), gpu.DeviceVector.from_host(w)
        out, total = gpu.cumulative_sums(v, with_total=True)
        where, sums, tot = gpu.prefix_search(v, [0.0, 1e3, -1e3, np.nan, 1e30])
        rel = gpu.prefix_search(W, levels, relative=True)
        return [bits(out.to_float32()), np.array([total]).view(np.uint64), bits(gpu.running_average(v).to_float32()), gpu.prefix_sums_at(v, pos).view(np.uint64),
                where, sums.view(np.uint64), np.array([tot]).view(np.uint64), rel[0], rel[1].view(np.uint64),
                gpu.weighted_quantiles(X, W, levels).view(np.uint64), np.array([gpu.weighted_expected_shortfall(X, W, 0.5)]).view(np.uint64),
                bits(gpu.expected_shortfall_curve(X).to_float32())]
    monkeypatch.setenv("FMHIP_DEVICE_PREFIX", "1")
    launches = gpu.pool_stats().n_kernel_launches
    device = everything()
    assert gpu.pool_stats().n_kernel_launches > launches
    monkeypatch.setenv("FMHIP_DEVICE_PREFIX", "0")
    host = everything()
    for k, (d, h) in enumerate(zip(device, host)):
        assert d.shape == h.shape and (d == h).all(), k


def test_small_large_small_on_one_engine(gpu):
    """The scratch and the pinned stage grow between the calls (4096 queries behind 3) and serve the small ones again."""
    rng = np.random.default_rng(12)
    small, large = dyadic(65, rng), dyadic(PAST, rng)
    vs, vl = gpu.DeviceVector.from_host(small), gpu.DeviceVector.from_host(large)
    ps, pl = np.cumsum(small, dtype=np.float64), np.cumsum(large, dtype=np.float64)
    many = rng.integers(0, PAST, MAXQ)
    for _ in range(2):
        assert same_f64(gpu.prefix_sums_at(vs, [0, 64, 3]), ps[[0, 64, 3]])
        assert same_f64(gpu.prefix_sums_at(vl, many), pl[many])
        assert (gpu.prefix_search(vl, pl[many])[0] == np.searchsorted(pl, pl[many], side="left")).all()
        assert (bits(gpu.cumulative_sums(vs).to_float32()) == bits(ps.astype(np.float32))).all()


# ---------------------------------------------------------------- the fronts: a device list, thread engines
_FRONTS = r'''
import ctypes as C, importlib, json, os, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode, out_path = sys.argv[1], sys.argv[2]
N = fm._native
n = 100_003
rng = np.random.default_rng(77)
a = ((10.0 ** rng.uniform(-8.0, 8.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
positions = np.array([0, n - 1, 17, 17, n // 2] + list(rng.integers(0, n, 295)), dtype=np.int64)
thresholds = np.array([0.0, 0.5, 1.0, -1.0, np.nan, 2.0])
res, info = {}, {}

def everything(tag, v):
    out, total = fm.cumulative_sums(v, with_total=True)
    res[tag + "_sums"], res[tag + "_total"] = out.to_float32(), np.array([total])
    res[tag + "_mean"] = fm.running_average(v).to_float32()
    res[tag + "_at"] = fm.prefix_sums_at(v, positions)
    where, sums, tot = fm.prefix_search(v, thresholds, relative=True)
    res[tag + "_where"], res[tag + "_found"], res[tag + "_tot"] = where, sums, np.array([tot])
    res[tag + "_in"] = v.to_float32()

if mode == "devices_one":
    fm.init_devices([0])
    fm.set_fusion(True)
    V = fm.DeviceVector.from_host(a)
    everything("stored", V)
    everything("pending", V.v1s1("MULT_S", 2.0))
elif mode == "devices_two":
    fm.init_devices([0, 0])
    lib = fm.lib()
    V = fm.DeviceVector.from_host(a)
    V.to_float32()
    before = fm.pool_stats()
    h, total = C.c_int64(0), C.c_double(-1.0)
    outd = (C.c_double * positions.size)(); where = (C.c_int64 * thresholds.size)()
    info["status"] = [lib.fmhip_prefix_sums(V.handle, 0, C.byref(h), C.byref(total)),
                      lib.fmhip_prefix_sums(V.handle, 1, C.byref(h), None),
                      lib.fmhip_prefix_sums_at(V.handle, positions.ctypes.data_as(C.POINTER(C.c_int64)), positions.size, outd),
                      lib.fmhip_prefix_search(V.handle, thresholds.ctypes.data_as(C.POINTER(C.c_double)), thresholds.size, 1, where, outd, C.byref(total))]
    info["unsupported"] = N.ERR_UNSUPPORTED
    info["message"] = lib.fmhip_last_error().decode("utf-8", "replace")
    after = fm.pool_stats()
    info["launches"] = [before.n_kernel_launches, after.n_kernel_launches]
    info["live"] = [before.n_live_vectors, after.n_live_vectors]
    info["outputs"] = [h.value, total.value]
    os.environ["FMHIP_DEVICE_PREFIX"] = "0"                  # the documented fallback: through reads and uploads, on any device list
    everything("host", V)
elif mode == "threads":
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    V = fm.DeviceVector.from_host(a)
    pend = V.v1s1("MULT_S", 2.0)                               # pending, owned by the main thread's engine
    kept = {}
    def other():
        kept["stored"] = fm.cumulative_sums(V, with_total=True)
        kept["mean"] = fm.running_average(pend)
        res["stored_at"] = fm.prefix_sums_at(V, positions)
        res["pending_at"] = fm.prefix_sums_at(pend, positions)
        where, sums, tot = fm.prefix_search(pend, thresholds, relative=True)
        res["pending_where"], res["pending_found"], res["pending_tot"] = where, sums, np.array([tot])
    t = threading.Thread(target=other); t.start(); t.join()
    res["stored_sums"], res["stored_total"] = kept["stored"][0].to_float32(), np.array([kept["stored"][1]])      # read back on the main thread
    res["pending_mean"] = kept["mean"].to_float32()
    res["stored_in"], res["pending_in"] = V.to_float32(), pend.to_float32()
    kept.clear()
np.savez(out_path, **res)
print("RESULT " + json.dumps(info))
fm.shutdown()
'''


def _run_front(tmp_path, mode):
    script = tmp_path / "fronts.py"
    script.write_text(_FRONTS % {"root": ROOT})
    out_path = tmp_path / (mode + ".npz")
    r = subprocess.run([sys.executable, str(script), mode, str(out_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return info, dict(np.load(out_path))


def _check_everything(gpu, res, tag, a, positions, thresholds):
    p = definition(gpu, a)
    assert same_f32(res[tag + "_sums"], rounded(p, False)) and same_f64(res[tag + "_total"], p[-1:]), tag
    assert same_f32(res[tag + "_mean"], rounded(p, True)), tag
    assert same_f64(res[tag + "_at"], p[positions]), tag
    want = [first_crossing(p, t) for t in thresholds * p[-1]]
    assert (res[tag + "_where"] == [w[0] for w in want]).all() and same_f64(res[tag + "_found"], [w[1] for w in want]) and same_f64(res[tag + "_tot"], p[-1:]), tag


@pytest.mark.parametrize("mode", ["devices_one", "devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  A device list of ONE shard is that shard's call: everything equals the definition, on stored and on pending
    operands.  A list of two answers FMHIP_ERR_UNSUPPORTED for the three calls — nothing launched, nothing left behind — and the mirror's
    host path (FMHIP_DEVICE_PREFIX=0) gives the definition's results there.  Thread engines: a thread that owns neither the vector nor the
    pending one scans them; the outputs are read on the main thread."""
    n = 100_003
    rng = np.random.default_rng(77)
    a = ((10.0 ** rng.uniform(-8.0, 8.0, n)) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    positions = np.array([0, n - 1, 17, 17, n // 2] + list(rng.integers(0, n, 295)), dtype=np.int64)
    thresholds = np.array([0.0, 0.5, 1.0, -1.0, np.nan, 2.0])
    doubled = (a * np.float32(2.0)).astype(np.float32)
    info, res = _run_front(tmp_path, mode)
    if mode == "devices_one":
        assert (bits(res["stored_in"]) == bits(a)).all() and (bits(res["pending_in"]) == bits(doubled)).all()
        _check_everything(gpu, res, "stored", a, positions, thresholds)
        _check_everything(gpu, res, "pending", doubled, positions, thresholds)
    elif mode == "devices_two":
        assert info["status"] == [info["unsupported"]] * 4 and info["unsupported"] == gpu._native.ERR_UNSUPPORTED
        assert "shards" in info["message"]
        assert info["launches"][0] == info["launches"][1] and info["live"][0] == info["live"][1] and info["outputs"] == [0, -1.0]
        assert (bits(res["host_in"]) == bits(a)).all()
        _check_everything(gpu, res, "host", a, positions, thresholds)
    else:
        assert (bits(res["stored_in"]) == bits(a)).all() and (bits(res["pending_in"]) == bits(doubled)).all()
        p, pd = definition(gpu, a), definition(gpu, doubled)
        assert same_f32(res["stored_sums"], rounded(p, False)) and same_f64(res["stored_total"], p[-1:]) and same_f64(res["stored_at"], p[positions])
        assert same_f32(res["pending_mean"], rounded(pd, True)) and same_f64(res["pending_at"], pd[positions])
        want = [first_crossing(pd, t) for t in thresholds * pd[-1]]
        assert (res["pending_where"] == [w[0] for w in want]).all() and same_f64(res["pending_found"], [w[1] for w in want]) and same_f64(res["pending_tot"], pd[-1:])
