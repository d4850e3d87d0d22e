"""Sort on the device (include/fmhip.h: fmhip_sort_by_key, fmhip_argsort, fmhip_rank_scores, fmhip_vec_read_elements)
through the C-ABI and the Python mirror.  A stable sort has one right answer: every check is an equality with the host definition
(fmhip_argsort_host, itself checked against numpy's stable argsort of the keys in tests/test_sort_cpu.py) or with numpy.  Sizes come from
the constants of csrc/sort_host.hpp, read from the header, and every large size asserts the regime it is there for — a full count table,
chunks of more than two tiles, a second trip of the gather's and the scores' grid-stride loop, a second chunk of the permutation's
read-back — so that a change of a constant fails an assert instead of testing nothing.  No test here asks the device for anything out of
range: bad arguments are refused on the host before a launch, and the largest n sorted is 2^24 + 3.  Sizes near 2^31 - 1 are covered by
the arithmetic checks of tests/cpp/test_sort_host.cpp alone."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_sort_cpu import argsort_host, byte_families, inputs, keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "sort_host.hpp")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_SORT_\w+) = ([^;]+);", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


K = header_constants()
TILE = K["FM_SORT_TILE"]
assert TILE == K["FM_SORT_BLOCK"] * K["FM_SORT_ITEMS"]


def chunk_tiles(n):
    tiles = -(-n // TILE)
    return max(K["FM_SORT_MIN_CHUNK_TILES"], -(-tiles // K["FM_SORT_MAX_BLOCKS"]))


def blocks(n):
    return -(-(-(-n // TILE)) // chunk_tiles(n))


CHUNK = chunk_tiles(1) * TILE                   # one workgroup's chunk while the table is not full
THREE = 2 * CHUNK + 1                           # the smallest n with three workgroups …
while THREE % TILE == 0 or THREE % 64 == 0: THREE += 1      # … (it is) and a ragged tail
assert blocks(THREE) == 3 and blocks(THREE - 1) == 2 and blocks(CHUNK) == 1 and blocks(CHUNK + 1) == 2
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, THREE, 100_003})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
def test_argsort_is_the_host_definition(gpu, n):
    rng = np.random.default_rng(n)
    for name, a in inputs(n, rng):
        v = gpu.DeviceVector.from_host(a)
        got = gpu.argsort(v)
        want = argsort_host(gpu, a)
        assert got.dtype == np.int64 and (got == want).all(), (name, n, int(np.flatnonzero(got != want)[0]))
        if name in ("constant", "all NaN"):
            assert (got == np.arange(n)).all(), (name, n)                     # stability
        assert (bits(v.to_float32()) == bits(a)).all(), (name, n)              # the input is unchanged


def test_argsort_of_a_million_and_three(gpu):
    n = (1 << 20) + 3
    rng = np.random.default_rng(11)
    for name, a in inputs(n, rng):
        if name not in ("normal", "payoff with signed zeros", "specials", "only byte 2 varies"): continue
        got = gpu.argsort(gpu.DeviceVector.from_host(a))
        assert (got == np.argsort(keys(a), kind="stable")).all(), name


@pytest.mark.parametrize("n", [1, 65, TILE + 1, THREE, 100_003])
@pytest.mark.parametrize("n_values", [0, 1, 8])
def test_sort_by_key_is_a_bit_copy_through_the_permutation(gpu, n, n_values):
    rng = np.random.default_rng(1000 * n_values + n)
    special = dict(inputs(n, rng))
    a = special["specials"].copy()
    a[::5] = np.where(rng.random(a[::5].size) < 0.5, np.float32(-0.0), np.float32(0.0))          # zeros of both signs among NaNs of several payloads
    companions = [special[name] for name in ("payoff with signed zeros", "specials", "uniform", "denormals", "normal", "clustered", "signed zeros", "all NaN")][:n_values]
    if n_values == 8:
        companions[7] = a                                                       # the key itself as a companion
        cb = bits(companions[1]).copy(); cb[::3] = 0xFFC00000 | (np.arange(cb[::3].size, dtype=np.uint32) & 0x3FFFFF); companions[1] = cb.view(np.float32)
    perm = argsort_host(gpu, a)
    key = gpu.DeviceVector.from_host(a)
    vals = [key if (n_values == 8 and i == 7) else gpu.DeviceVector.from_host(c) for i, c in enumerate(companions)]
    sk, sv = gpu.sort_by_key(key, vals)
    assert sk.n == n and len(sv) == n_values
    assert (bits(sk.to_float32()) == bits(a)[perm]).all()
    for c, out in zip(companions, sv):
        assert (bits(out.to_float32()) == bits(c)[perm]).all()
    assert (bits(key.to_float32()) == bits(a)).all()                            # inputs unchanged
    for c, v in zip(companions, vals):
        assert (bits(v.to_float32()) == bits(c)).all()


def test_pending_operands_give_the_bits_of_materialised_ones(gpu, oracle):
    n = THREE
    rng = np.random.default_rng(3)
    a = rng.standard_normal(n).astype(np.float32)
    c = rng.random(n, dtype=np.float32)
    prev = gpu.set_fusion(True)
    try:
        A, Cv = gpu.DeviceVector.from_host(a), gpu.DeviceVector.from_host(c)
        before = gpu.pool_stats().n_kernel_launches
        pk, pc = A.v1s1("MULT_S", 2.0).v1s1("ADD_S", 1.0), Cv.v1s1("MULT_S", 3.0)      # pending, fused
        assert gpu.pool_stats().n_kernel_launches == before
        sk, (sc,) = gpu.sort_by_key(pk, [pc])
        mk, mc = gpu.DeviceVector.from_host(pk.to_float32()), gpu.DeviceVector.from_host(pc.to_float32())
        rk, (rc,) = gpu.sort_by_key(mk, [mc])
        assert (bits(sk.to_float32()) == bits(rk.to_float32())).all() and (bits(sc.to_float32()) == bits(rc.to_float32())).all()
        want_key = oracle.f_v1s1("ADD_S", oracle.f_v1s1("MULT_S", a, 2.0), 1.0)
        perm = argsort_host(gpu, want_key)
        assert (bits(sk.to_float32()) == bits(want_key)[perm]).all()
        assert (bits(sc.to_float32()) == bits(oracle.f_v1s1("MULT_S", c, 3.0))[perm]).all()
        assert (gpu.argsort(A.v1s1("MULT_S", 2.0).v1s1("ADD_S", 1.0)) == perm).all()
    finally:
        gpu.set_fusion(prev)


@pytest.mark.parametrize("n", [1, 64, TILE - 1, THREE, 100_003])
def test_rank_scores_are_the_ordinal_ranks(gpu, n):
    rng = np.random.default_rng(n + 1)
    for name, a in inputs(n, rng):
        if name not in ("normal", "payoff", "constant", "specials", "only byte 0 varies"): continue
        perm = argsort_host(gpu, a)
        inverse = np.empty(n, dtype=np.int64); inverse[perm] = np.arange(n)
        got = gpu.rank_scores(gpu.DeviceVector.from_host(a)).to_float32()
        assert (bits(got) == bits(((inverse + 0.5) / n).astype(np.float32))).all(), (name, n)


@pytest.mark.parametrize("n", [2, 3, 100, THREE, 100_003])
def test_sorted_quantiles_are_getQuantile_level_by_level(gpu, n):
    rng = np.random.default_rng(n + 2)
    d = np.maximum(rng.standard_normal(n) - 0.2, 0.0) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    x = gpu.RandomVariableHipFactory().createRandomVariable(0.0, d)
    levels = [0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0]
    got = gpu.sorted_quantiles(x, levels)
    want = np.array([x.getQuantile(q) for q in levels])
    assert got.dtype == np.float64 and (got.view(np.uint64) == want.view(np.uint64)).all(), (got, want)


def test_spearman_matrix(gpu):
    """The reference is numpy's correlation matrix of the SAME ordinal ranks (ties by path index), taken as the rank scores the call is
    defined on — (rank + 0.5) / n in fp32, exact inputs of both — and agrees to 1e-12: what is left is the order of fp64 additions.
    Against the correlation of the integer ranks themselves the scores' rounding to fp32 (relative 2^-24 each) shows: a bound of
    4 · 2^-24 / (1/12) < 3e-6 on a variance of 1/12 holds for any n and is asserted beside it."""
    n = 20_011
    rng = np.random.default_rng(9)
    z = rng.standard_normal((3, n))
    data = [z[0], 0.6 * z[0] + 0.8 * z[1], np.maximum(z[2] - 0.2, 0.0)]        # the third: half ties
    vs = [gpu.DeviceVector.from_host(np.float32(x)) for x in data]
    got = gpu.spearman_matrix(vs)
    ranks = []
    for x in data:
        perm = argsort_host(gpu, np.float32(x))
        inverse = np.empty(n, dtype=np.int64); inverse[perm] = np.arange(n)
        ranks.append(inverse)
    scores = [((r + 0.5) / n).astype(np.float32).astype(np.float64) for r in ranks]
    want = np.corrcoef(np.array(scores))
    print("spearman: max difference to numpy on the scores", np.abs(got - want).max(), "to numpy on the integer ranks", np.abs(got - np.corrcoef(np.array(ranks, dtype=np.float64))).max())
    assert got.shape == (3, 3) and (np.diag(got) == 1.0).all()
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(got - np.corrcoef(np.array(ranks, dtype=np.float64))).max() <= 3e-6
    assert (got == got.T).all()


def test_read_elements_is_the_indexed_download(gpu):
    n = THREE
    a = dict(inputs(n, np.random.default_rng(4)))["specials"]
    v = gpu.DeviceVector.from_host(a)
    positions = np.array([0, n - 1, 17, 17, n // 2, 0, CHUNK, TILE - 1], dtype=np.int64)
    got = gpu.read_elements(v, positions)
    want = a[positions].astype(np.float64)
    assert (got.view(np.uint64) == want.view(np.uint64)).all() or ((np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(got)] == want[~np.isnan(want)]).all())
    one = gpu.read_elements(gpu.DeviceVector.from_host(np.float32([-0.0])), [0])
    assert one[0] == 0.0 and np.signbit(one[0])


def test_refusals_are_made_on_the_host(gpu):
    N = gpu._native
    lib = gpu.lib()
    n = 1000
    v = gpu.DeviceVector.from_host(np.arange(n, dtype=np.float32))
    short = gpu.DeviceVector.from_host(np.arange(n - 1, dtype=np.float32))
    before = gpu.pool_stats().n_kernel_launches
    out_key, out_vals = C.c_int64(0), (C.c_int64 * 9)()
    nine = (C.c_int64 * 9)(*([v.handle] * 9))
    assert lib.fmhip_sort_by_key(v.handle, nine, 9, C.byref(out_key), out_vals) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_sort_by_key(v.handle, nine, -1, C.byref(out_key), out_vals) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_sort_by_key(v.handle, None, 0, None, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_sort_by_key(v.handle, None, 1, C.byref(out_key), out_vals) == N.ERR_INVALID_ARGUMENT
    two = (C.c_int64 * 2)(v.handle, short.handle)
    assert lib.fmhip_sort_by_key(v.handle, two, 2, C.byref(out_key), out_vals) == N.ERR_SIZE_MISMATCH
    assert lib.fmhip_sort_by_key(v.handle + 12345, None, 0, C.byref(out_key), None) == N.ERR_INVALID_HANDLE
    assert lib.fmhip_argsort(v.handle, None) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_rank_scores(v.handle, None) == N.ERR_INVALID_ARGUMENT
    out = (C.c_double * 3)()
    for bad in ([-1], [n], [0, 5, n], [1 << 40]):
        p = np.array(bad, dtype=np.int64)
        assert lib.fmhip_vec_read_elements(v.handle, p.ctypes.data_as(C.POINTER(C.c_int64)), p.size, out) == N.ERR_INVALID_ARGUMENT, bad
    p = np.zeros(1, dtype=np.int64)
    assert lib.fmhip_vec_read_elements(v.handle, p.ctypes.data_as(C.POINTER(C.c_int64)), 0, out) == N.ERR_INVALID_ARGUMENT
    assert lib.fmhip_vec_read_elements(v.handle, None, 1, out) == N.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gpu.sort_by_key(v, [short])
    # a communicator of two ranks: a global order needs an exchange of elements, which is not done
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        perm = np.zeros(n, dtype=np.int64)
        assert lib.fmhip_argsort(v.handle, perm.ctypes.data_as(C.POINTER(C.c_int64))) == N.ERR_UNSUPPORTED
        assert lib.fmhip_rank_scores(v.handle, C.byref(out_key)) == N.ERR_UNSUPPORTED
        assert lib.fmhip_sort_by_key(v.handle, None, 0, C.byref(out_key), None) == N.ERR_UNSUPPORTED
    finally:
        gpu.set_expectation_comm(1, 0, None)
    assert gpu.pool_stats().n_kernel_launches == before                          # nothing was launched for any of it
    assert (gpu.argsort(v) == np.arange(n)).all()


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
        ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 5)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for y in ys:
            try:
                y.to_float32()
                read_error = None
            except gpu.FmhipError as e:
                read_error = e.code
                assert "given up" in str(e)
            calls = (lambda: gpu.argsort(y), lambda: gpu.sort_by_key(base, [y]), lambda: gpu.rank_scores(y), lambda: gpu.read_elements(y, [0]))
            for call in calls:
                if read_error is None:
                    call()
                else:
                    with pytest.raises(gpu.FmhipError) as info:
                        call()
                    assert info.value.code == read_error == gpu._native.ERR_INVALID_ARGUMENT and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


def test_the_host_switch_gives_identical_results(gpu, monkeypatch):
    n = THREE
    a = dict(inputs(n, np.random.default_rng(6)))["specials"]
    c = np.random.default_rng(7).standard_normal(n).astype(np.float32)
    levels = [0.0, 0.1, 0.5, 0.9, 1.0]
    def everything():
        key, comp = gpu.DeviceVector.from_host(a), gpu.DeviceVector.from_host(c)
        sk, (sc,) = gpu.sort_by_key(key, [comp])
        return [gpu.argsort(key), bits(sk.to_float32()), bits(sc.to_float32()), bits(gpu.rank_scores(key).to_float32()),
                gpu.sorted_quantiles(comp, levels).view(np.uint64), gpu.spearman_matrix([key, comp]).view(np.uint64)]
    monkeypatch.setenv("FMHIP_DEVICE_SORT", "1")
    launches = gpu.pool_stats().n_kernel_launches
    device = everything()
    assert gpu.pool_stats().n_kernel_launches > launches
    monkeypatch.setenv("FMHIP_DEVICE_SORT", "0")
    host = everything()
    for d, h in zip(device, host):
        assert d.shape == h.shape and (d == h).all()


def test_the_ping_pong_buffers_go_back_to_the_pool(gpu):
    n = 100_003
    a = np.random.default_rng(8).standard_normal(n).astype(np.float32)
    key, comp = gpu.DeviceVector.from_host(a), gpu.DeviceVector.from_host(a[::-1].copy())
    gpu.argsort(key); gpu.sort_by_key(key, [comp]); gpu.rank_scores(key); gpu.read_elements(key, [0])       # warm: scratch and pinned blocks are the engine's for good
    before = gpu.pool_stats().bytes_in_use
    probe = gpu.DeviceVector.from_host(a)
    per_vector = gpu.pool_stats().bytes_in_use - before          # what one vector of n takes from the pool
    del probe
    assert per_vector >= 4 * n
    for call, n_out in ((lambda: gpu.argsort(key), 0), (lambda: gpu.sort_by_key(key, [comp]), 2), (lambda: gpu.rank_scores(key), 1), (lambda: gpu.read_elements(key, [0, n - 1]), 0)):
        before = gpu.pool_stats()
        kept = call()
        after = gpu.pool_stats()
        assert after.n_live_vectors - before.n_live_vectors == n_out
        assert after.bytes_in_use - before.bytes_in_use == n_out * per_vector, (after.bytes_in_use - before.bytes_in_use, n_out)
        del kept


# ---------------------------------------------------------------- past the sizes at which the grids stop growing
STREAM = 4 * 256 * K["FM_SORT_STREAM_MAX_BLOCKS"]           # elements of one trip of the gather's and the scores' grid-stride loop
READBACK = K["FM_SORT_READBACK_CHUNK"]                      # elements of the permutation per D2H copy of fmhip_argsort
FULL = K["FM_SORT_MAX_BLOCKS"] * K["FM_SORT_MIN_CHUNK_TILES"] * TILE      # 4 194 304: the count table is full at the smallest chunk
N_CHUNK3 = FULL + 1                                         # 4 194 305: the first n with a chunk of three tiles
N_BOTH = 3 * FULL // 2                                      # 6 291 456: a chunk of three tiles AND a full table
N_CLIP = FULL + TILE + 1                                    # 4 196 353: a chunk of three tiles that the end of the vector clips to one
N_TRIP = STREAM + 100_003                                   # 8 488 611: a second, ragged trip of the gather and the scores
N_READBACK = READBACK + 3                                   # 16 777 219: a second D2H chunk, of three elements


def tiles(n):
    return -(-n // TILE)


def last_chunk_tiles(n):
    return tiles(n) - (blocks(n) - 1) * chunk_tiles(n)


def stream_trips(n):
    quads = -(-n // 4)
    grid = min(max(-(-quads // 256), 1), K["FM_SORT_STREAM_MAX_BLOCKS"])
    return -(-quads // (grid * 256))


# the regimes the sizes are there for (with today's constants: 1024 / 683 / 1024 / 684 / 829 / 911 workgroups, chunks of 2 / 3 / 3 / 3 / 5 / 9 tiles)
assert blocks(FULL) == K["FM_SORT_MAX_BLOCKS"] and chunk_tiles(FULL) == K["FM_SORT_MIN_CHUNK_TILES"] == 2 and last_chunk_tiles(FULL) == 2
assert chunk_tiles(N_CHUNK3) == 3 and blocks(N_CHUNK3) % 4 == 3 and blocks(N_CHUNK3) < K["FM_SORT_MAX_BLOCKS"]
assert last_chunk_tiles(N_CHUNK3) == 3 and N_CHUNK3 % TILE == 1      # the run carries over three tiles in every workgroup; the last tile holds one element
assert chunk_tiles(N_BOTH) == 3 and blocks(N_BOTH) == K["FM_SORT_MAX_BLOCKS"] and blocks(N_BOTH) % 4 == 0
assert chunk_tiles(N_CLIP) == 3 and last_chunk_tiles(N_CLIP) == 1 and blocks(N_CLIP) % 4 == 0      # t1 = min(t0 + chunk, tiles) clips a chunk of three
assert all(stream_trips(n) == 1 for n in (FULL, N_CHUNK3, N_BOTH, N_CLIP, STREAM)) and all(n <= READBACK for n in (FULL, N_CHUNK3, N_BOTH, N_CLIP, N_TRIP))
assert stream_trips(N_TRIP) == 2 and -(-N_TRIP // 4) % 256 != 0 and chunk_tiles(N_TRIP) > 3 and blocks(N_TRIP) % 4 == 1
assert stream_trips(N_READBACK) == 3 and -(-N_READBACK // READBACK) == 2 and N_READBACK - READBACK == 3
assert chunk_tiles(N_READBACK) > 3 and 2 < last_chunk_tiles(N_READBACK) < chunk_tiles(N_READBACK) and blocks(N_READBACK) % 4 == 3      # a clipped chunk longer than two tiles
assert N_READBACK <= 0x7fffffff

FAMILIES = ("normal", "specials", "constant", "two values") + tuple(f"only byte {b} varies" for b in range(4))
LARGE = [(n, f) for n in (FULL, N_CHUNK3, N_BOTH) for f in FAMILIES] + [(n, f) for n in (N_CLIP, N_TRIP, N_READBACK) for f in ("normal", "specials")]
_SHARED = {("normal", N_CHUNK3): None, ("normal", N_TRIP): None, ("specials", N_TRIP): None, ("normal", N_READBACK): None}      # used by more than one test: built once


def _family(name, n):
    """One family of test_sort_cpu.inputs at a large n, built directly (not all fifteen)."""
    rng = np.random.default_rng(n % 1_000_003 + 7 * FAMILIES.index(name))
    if name == "normal": return rng.standard_normal(n, dtype=np.float32)
    if name == "constant": return np.full(n, 1.25, dtype=np.float32)
    if name == "two values": return np.where(rng.random(n, dtype=np.float32) < 0.3, np.float32(-3.5), np.float32(7.0)).astype(np.float32)
    if name == "specials":
        a = rng.standard_normal(n, dtype=np.float32)
        a[::7] = np.inf; a[3::11] = -np.inf
        u = a.view(np.uint32)
        u[5::13] = 0x7FC00000; u[6::17] = 0xFFC00001; u[1::19] = 0x7F800123      # NaNs of both signs, several payloads
        return a
    return dict(byte_families(n, rng))[name]


def large(fm, name, n):
    """(input, the definition's permutation), read-only; shared between the tests that use the same one."""
    if _SHARED.get((name, n)) is not None: return _SHARED[(name, n)]
    a = _family(name, n)
    perm = argsort_host(fm, a)
    a.setflags(write=False); perm.setflags(write=False)
    if (name, n) in _SHARED: _SHARED[(name, n)] = (a, perm)
    return a, perm


@pytest.fixture(scope="module", autouse=True)
def _shared_inputs_end_with_the_module():
    yield
    for k in _SHARED: _SHARED[k] = None


def check_order(got, a, tag):
    """O(n), without a second sort: a permutation, ascending in the key, equal keys in ascending path order."""
    n = a.size
    assert got.dtype == np.int64 and got.shape == (n,) and got.min() >= 0 and got.max() < n, tag
    assert (np.bincount(got, minlength=n) == 1).all(), tag
    k = keys(a)[got]
    assert (k[1:] >= k[:-1]).all(), (tag, "not ascending at", int(np.flatnonzero(k[1:] < k[:-1])[0]))
    tie = k[1:] == k[:-1]
    assert (got[1:][tie] > got[:-1][tie]).all(), (tag, "unstable")


def f64(a):
    with np.errstate(invalid="ignore"):                      # (a signalling NaN among the specials)
        return np.asarray(a, dtype=np.float32).astype(np.float64)


def doubled(a):
    with np.errstate(invalid="ignore"):
        return (np.asarray(a, dtype=np.float32) * np.float32(2.0)).astype(np.float32)


def same_f64(got, want):
    nan = np.isnan(want)
    return got.dtype == np.float64 and (np.isnan(got) == nan).all() and (got.view(np.uint64)[~nan] == want.view(np.uint64)[~nan]).all()


@pytest.mark.parametrize("n,name", LARGE, ids=[f"{n}-{f.replace(' ', '_')}" for n, f in LARGE])
def test_argsort_of_millions_is_the_definition(gpu, n, name):
    a, want = large(gpu, name, n)
    v = gpu.DeviceVector.from_host(a)
    got = gpu.argsort(v)
    check_order(got, a, (name, n))
    assert (got == want).all(), (name, n, int(np.flatnonzero(got != want)[0]))
    if name == "constant":
        assert (got == np.arange(n)).all()                   # every workgroup's first destination is w · chunk
    if name == "specials":
        nan = np.flatnonzero(np.isnan(a))
        assert nan.size > n // 20 and (got[n - nan.size:] == nan).all()      # every NaN last, in path order
    if (name, n) == ("normal", N_CHUNK3):
        assert (got == np.argsort(keys(a), kind="stable")).all()
    if n in (FULL, N_READBACK):
        assert (bits(v.to_float32()) == bits(a)).all()          # the input is unchanged


def test_sort_by_key_of_nine_vectors_on_the_second_trip(gpu):
    n = N_TRIP
    a, perm = large(gpu, "specials", n)
    rng = np.random.default_rng(12)
    companions = [rng.random(n, dtype=np.float32) for _ in range(3)] + [large(gpu, "normal", n)[0], -a]
    payloads = (np.uint32(0xFFC00000) | (np.arange(n, dtype=np.uint32) & np.uint32(0x3FFFFF))).view(np.float32)       # a NaN of its own payload per path
    zeros = np.where(companions[0] < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    companions += [payloads, zeros, a]                        # the key itself as the eighth companion
    key = gpu.DeviceVector.from_host(a)
    vals = [gpu.DeviceVector.from_host(c) for c in companions[:7]] + [key]
    sk, sv = gpu.sort_by_key(key, vals)
    assert sk.n == n and len(sv) == 8
    assert (bits(sk.to_float32()) == bits(a)[perm]).all()
    for i, (c, out) in enumerate(zip(companions, sv)):
        assert (bits(out.to_float32()) == bits(c)[perm]).all(), i
    del sk, sv
    for i, (c, v) in enumerate(zip(companions, vals)):        # the inputs are unchanged (the eighth is the key)
        assert (bits(v.to_float32()) == bits(c)).all(), i


@pytest.mark.parametrize("n", [N_TRIP, N_READBACK])
def test_rank_scores_of_millions(gpu, n):
    a, perm = large(gpu, "normal", n)
    inverse = np.empty(n, dtype=np.int64); inverse[perm] = np.arange(n)
    got = gpu.rank_scores(gpu.DeviceVector.from_host(a)).to_float32()
    assert (bits(got) == bits(((inverse + 0.5) / n).astype(np.float32))).all()


def _positions(n, count, seed):
    """Random with repeats; n - 1 and 0 among them (count 1: n - 1)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, n, count, dtype=np.int64)
    p[count // 2:] = p[: count - count // 2]                  # every position of the first half a second time
    p[0] = n - 1
    if count > 1: p[-1] = 0
    return p


@pytest.mark.parametrize("count", [1, 256, 257, 100_003])
def test_read_elements_with_more_than_one_workgroup(gpu, count):
    n = N_TRIP
    a, _ = large(gpu, "specials", n)
    v = gpu.DeviceVector.from_host(a)
    positions = _positions(n, count, count)
    assert positions.max() == n - 1 and (count == 1 or positions.min() == 0) and (count < 4 or np.unique(positions).size < count)
    got = gpu.read_elements(v, positions)
    assert got.shape == (count,) and same_f64(got, f64(a[positions]))


def test_a_thousand_and_one_sorted_quantiles(gpu):
    n = 100_003
    rng = np.random.default_rng(n + 3)
    d = np.maximum(rng.standard_normal(n) - 0.2, 0.0) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    x = gpu.RandomVariableHipFactory().createRandomVariable(0.0, d)
    levels = np.linspace(0.0, 1.0, 1001)
    got = gpu.sorted_quantiles(x, levels)
    want = np.array([x.getQuantile(float(q)) for q in levels])
    assert got.dtype == np.float64 and (got.view(np.uint64) == want.view(np.uint64)).all()


def test_small_large_small_on_one_engine(gpu):
    """The count table (side-pass scratch) and the pinned stage grow for the large call and the read of 100 003 elements and serve the small
    calls behind them; the ping-pong buffers go back to the pool every time."""
    small = np.random.default_rng(65).integers(-3, 4, 65).astype(np.float32)
    a, perm = large(gpu, "normal", N_CHUNK3)
    vs, vb = gpu.DeviceVector.from_host(small), gpu.DeviceVector.from_host(a)
    positions = _positions(N_CHUNK3, 100_003, 5)
    want_small, want_read = argsort_host(gpu, small), f64(a[positions])
    before = gpu.pool_stats()
    for step in range(2):
        assert (gpu.argsort(vs) == want_small).all(), step
        assert same_f64(gpu.read_elements(vb, positions), want_read), step
        got = gpu.argsort(vb)
        assert (got == perm).all(), step
        del got
        assert same_f64(gpu.read_elements(vb, positions[:300]), want_read[:300]), step
        assert (gpu.argsort(vs) == want_small).all(), step
    after = gpu.pool_stats()
    assert after.bytes_in_use == before.bytes_in_use and after.n_live_vectors == before.n_live_vectors


def test_a_slab_view_is_a_key(gpu):
    """The views of a Brownian motion's slab do not start at their allocation's start: the count kernel's 16-byte loads and the gather's whole
    quads meet a neighbour there.  10 001 paths: no multiple of four."""
    paths, factors, steps = 10_001, 2, 2
    bm = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, steps, 0.5), factors, paths, 4711)
    views = [[bm.getBrownianIncrement(t, f).realizations for f in range(factors)] for t in range(steps)]
    host = [[v.to_float32().copy() for v in row] for row in views]
    for t in range(steps):
        for f in range(factors):
            got = gpu.argsort(views[t][f])
            assert (got == argsort_host(gpu, host[t][f])).all(), (t, f)
            sk, (sc,) = gpu.sort_by_key(views[t][f], [views[steps - 1 - t][f]])
            assert (bits(sk.to_float32()) == bits(host[t][f])[got]).all() and (bits(sc.to_float32()) == bits(host[steps - 1 - t][f])[got]).all(), (t, f)
            score = gpu.rank_scores(views[t][f]).to_float32()
            inverse = np.empty(paths, dtype=np.int64); inverse[got] = np.arange(paths)
            assert (bits(score) == bits(((inverse + 0.5) / paths).astype(np.float32))).all(), (t, f)
            for tt in range(steps):
                for ff in range(factors):
                    assert (bits(views[tt][ff].to_float32()) == bits(host[tt][ff])).all(), (t, f, tt, ff)      # every view, the neighbours among them, is unchanged


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
key = rng.standard_normal(n).astype(np.float32)
key[::7] = np.inf; key[3::11] = -np.inf
u = key.view(np.uint32); u[5::13] = 0x7FC00000; u[6::17] = 0xFFC00001; u[1::19] = 0x7F800123
comp = rng.standard_normal(n).astype(np.float32)
own = rng.random(n, dtype=np.float32)
positions = np.array([0, n - 1, 17, 17, n // 2] + list(rng.integers(0, n, 295)), dtype=np.int64)
levels = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]
res, info = {}, {}

def everything(tag, k, c):
    res[tag + "_argsort"] = fm.argsort(k)
    sk, (s1, s2) = fm.sort_by_key(k, [c, k])
    res[tag + "_key"], res[tag + "_c"], res[tag + "_k2"] = sk.to_float32(), s1.to_float32(), s2.to_float32()
    res[tag + "_scores"] = fm.rank_scores(k).to_float32()
    res[tag + "_read"] = fm.read_elements(k, positions)
    res[tag + "_quantiles"] = fm.sorted_quantiles(c, levels)
    res[tag + "_spearman"] = fm.spearman_matrix([k, c])
    res[tag + "_key_in"], res[tag + "_c_in"] = k.to_float32(), c.to_float32()

if mode == "devices_one":
    fm.init_devices([0])
    fm.set_fusion(True)
    K, Cv = fm.DeviceVector.from_host(key), fm.DeviceVector.from_host(comp)
    everything("stored", K, Cv)
    everything("pending", K.v1s1("MULT_S", 2.0), Cv.v1s1("MULT_S", 2.0))
elif mode == "devices_two":
    fm.init_devices([0, 0])
    lib = fm.lib()
    K, Cv = fm.DeviceVector.from_host(key), fm.DeviceVector.from_host(comp)
    K.to_float32(); Cv.to_float32()
    before = fm.pool_stats()
    perm = np.full(n, -1, dtype=np.int64)
    h, hs, two = C.c_int64(0), (C.c_int64 * 2)(), (C.c_int64 * 2)(Cv.handle, K.handle)
    outd = (C.c_double * positions.size)()
    info["status"] = [lib.fmhip_argsort(K.handle, perm.ctypes.data_as(C.POINTER(C.c_int64))),
                      lib.fmhip_sort_by_key(K.handle, two, 2, C.byref(h), hs),
                      lib.fmhip_sort_by_key(K.handle, None, 0, C.byref(h), None),
                      lib.fmhip_rank_scores(K.handle, C.byref(h)),
                      lib.fmhip_vec_read_elements(K.handle, positions.ctypes.data_as(C.POINTER(C.c_int64)), positions.size, outd)]
    info["unsupported"] = N.ERR_UNSUPPORTED
    info["message"] = lib.fmhip_last_error().decode("utf-8", "replace")
    after = fm.pool_stats()
    info["launches"] = [before.n_kernel_launches, after.n_kernel_launches]
    info["live"] = [before.n_live_vectors, after.n_live_vectors]
    info["handles"] = [h.value, hs[0], hs[1]]
    info["perm_untouched"] = bool((perm == -1).all())
    res["select"] = K.select_ranks([0, 5, n // 2])
    m = Cv.moments()
    res["moments"] = np.array([m.sum, m.sumsq, m.min, m.max])
    os.environ["FMHIP_DEVICE_SORT"] = "0"                    # the documented fallback: through reads and uploads, on any device list
    res["host_argsort"] = fm.argsort(K)
    sk, (s1, s2) = fm.sort_by_key(K, [Cv, K])
    res["host_key"], res["host_c"], res["host_k2"] = sk.to_float32(), s1.to_float32(), s2.to_float32()
    res["host_scores"] = fm.rank_scores(K).to_float32()
    res["key_in"], res["c_in"] = K.to_float32(), Cv.to_float32()
elif mode == "threads":
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    K, Cv = fm.DeviceVector.from_host(key), fm.DeviceVector.from_host(comp)
    pend = Cv.v1s1("MULT_S", 2.0)                              # pending, owned by the main thread's engine
    kept = {}
    def other():
        mine = fm.DeviceVector.from_host(own)                  # owned by this thread's engine
        kept["sorted"] = fm.sort_by_key(K, [pend, mine])
        res["argsort"] = fm.argsort(K)
        kept["scores"] = fm.rank_scores(K)
        res["read"] = fm.read_elements(K, positions)
        res["read_pending"] = fm.read_elements(pend, positions)
        kept["mine"] = mine
    t = threading.Thread(target=other); t.start(); t.join()
    sk, (s1, s2) = kept["sorted"]                               # read back on the main thread
    res["key"], res["c"], res["own"], res["scores"] = sk.to_float32(), s1.to_float32(), s2.to_float32(), kept["scores"].to_float32()
    res["key_in"], res["c_in"], res["own_in"] = K.to_float32(), pend.to_float32(), kept["mine"].to_float32()
    kept.clear(); del sk, s1, s2
else:
    # a fresh engine: its side-pass scratch and pinned stage are at their smallest before the first call and grow between the calls
    fm.init(0)
    small = np.random.default_rng(65).integers(-3, 4, 65).astype(np.float32)
    big_n = int(sys.argv[3])
    big = np.random.default_rng(big_n %% 1_000_003).standard_normal(big_n, dtype=np.float32)      # the parent's "normal" of this size
    vs, vb = fm.DeviceVector.from_host(small), fm.DeviceVector.from_host(big)
    far = np.random.default_rng(5).integers(0, big_n, 100_003, dtype=np.int64)
    before = fm.pool_stats()
    res["small_0"] = fm.argsort(vs)
    res["read_0"] = fm.read_elements(vb, far)
    res["large"] = fm.argsort(vb)
    res["read_1"] = fm.read_elements(vb, far)
    res["small_1"] = fm.argsort(vs)
    after = fm.pool_stats()
    info["bytes"] = [before.bytes_in_use, after.bytes_in_use]
    info["live"] = [before.n_live_vectors, after.n_live_vectors]
np.savez(out_path, **res)
print("RESULT " + json.dumps(info))
fm.shutdown()
'''


def _front_inputs():
    n = 100_003
    rng = np.random.default_rng(77)
    key = rng.standard_normal(n).astype(np.float32)
    key[::7] = np.inf; key[3::11] = -np.inf
    u = key.view(np.uint32); u[5::13] = 0x7FC00000; u[6::17] = 0xFFC00001; u[1::19] = 0x7F800123
    comp = rng.standard_normal(n).astype(np.float32)
    own = rng.random(n, dtype=np.float32)
    positions = np.array([0, n - 1, 17, 17, n // 2] + list(rng.integers(0, n, 295)), dtype=np.int64)
    return n, key, comp, own, positions


def _run_front(tmp_path, mode, *more):
    script = tmp_path / "fronts.py"
    script.write_text(_FRONTS % {"root": ROOT})
    out_path = tmp_path / (mode + ".npz")
    r = subprocess.run([sys.executable, str(script), mode, str(out_path)] + [str(m) for m in more], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return info, dict(np.load(out_path))


def _scores(perm):
    inverse = np.empty(perm.size, dtype=np.int64); inverse[perm] = np.arange(perm.size)
    return ((inverse + 0.5) / perm.size).astype(np.float32)


@pytest.mark.parametrize("mode", ["devices_one", "devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  A device list of ONE shard is that shard's call: everything equals the definition, on stored and on pending
    operands.  A list of two answers FMHIP_ERR_UNSUPPORTED for the four calls — nothing launched, nothing left behind, the vectors as good
    as before — and the mirror's host path (FMHIP_DEVICE_SORT=0) gives the definition's results there.  Thread engines: a thread that owns
    neither the key nor the pending companion sorts them with a companion of its own; the outputs are read on the main thread."""
    n, key, comp, own, positions = _front_inputs()
    info, res = _run_front(tmp_path, mode)
    perm = argsort_host(gpu, key)
    if mode == "devices_one":
        for tag in ("stored", "pending"):
            k_in, c_in = res[tag + "_key_in"], res[tag + "_c_in"]
            if tag == "stored": assert (bits(k_in) == bits(key)).all() and (bits(c_in) == bits(comp)).all()
            else: assert (bits(c_in) == bits(doubled(comp))).all() and (keys(k_in) == keys(doubled(key))).all()       # (a NaN's payload after a multiplication is the device's)
            p = argsort_host(gpu, k_in)
            assert (res[tag + "_argsort"] == p).all(), tag
            assert (bits(res[tag + "_key"]) == bits(k_in)[p]).all() and (bits(res[tag + "_k2"]) == bits(k_in)[p]).all(), tag
            assert (bits(res[tag + "_c"]) == bits(c_in)[p]).all(), tag
            assert (bits(res[tag + "_scores"]) == bits(_scores(p))).all(), tag
            assert same_f64(res[tag + "_read"], f64(k_in[positions])), tag
            # the same calls on the session's single engine
            kv, cv = gpu.DeviceVector.from_host(k_in), gpu.DeviceVector.from_host(c_in)
            levels = [0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0]
            assert (res[tag + "_quantiles"].view(np.uint64) == gpu.sorted_quantiles(cv, levels).view(np.uint64)).all(), tag
            assert (res[tag + "_spearman"].view(np.uint64) == gpu.spearman_matrix([kv, cv]).view(np.uint64)).all(), tag
    elif mode == "devices_two":
        assert info["status"] == [info["unsupported"]] * 5 and info["unsupported"] == gpu._native.ERR_UNSUPPORTED
        assert "shards" in info["message"]
        assert info["launches"][0] == info["launches"][1] and info["live"][0] == info["live"][1]
        assert info["handles"] == [0, 0, 0] and info["perm_untouched"]
        assert (bits(res["key_in"]) == bits(key)).all() and (bits(res["c_in"]) == bits(comp)).all()
        assert same_f64(res["select"], f64(key[perm][[0, 5, n // 2]]))
        c64 = comp.astype(np.float64)
        s, ss, lo, hi = res["moments"]
        assert lo == c64.min() and hi == c64.max()
        assert abs(s - c64.sum()) <= 1e-12 * np.abs(c64).sum() and abs(ss - (c64 * c64).sum()) <= 1e-12 * (c64 * c64).sum()
        assert (res["host_argsort"] == perm).all()
        assert (bits(res["host_key"]) == bits(key)[perm]).all() and (bits(res["host_k2"]) == bits(key)[perm]).all() and (bits(res["host_c"]) == bits(comp)[perm]).all()
        assert (bits(res["host_scores"]) == bits(_scores(perm))).all()
    else:
        assert (bits(res["key_in"]) == bits(key)).all() and (bits(res["c_in"]) == bits(doubled(comp))).all() and (bits(res["own_in"]) == bits(own)).all()
        assert (res["argsort"] == perm).all()
        assert (bits(res["key"]) == bits(key)[perm]).all() and (bits(res["c"]) == bits(doubled(comp))[perm]).all() and (bits(res["own"]) == bits(own)[perm]).all()
        assert (bits(res["scores"]) == bits(_scores(perm))).all()
        assert same_f64(res["read"], f64(key[positions])) and same_f64(res["read_pending"], f64(doubled(comp)[positions]))


def test_scratch_and_stage_grow_on_a_fresh_engine(gpu, tmp_path):
    """test_small_large_small_on_one_engine on an engine that has run nothing yet (a process of its own): the first call finds the scratch and
    the stage at their smallest, the read of 100 003 elements and the sort of FULL + 1 make both grow, the small call behind them is right."""
    info, res = _run_front(tmp_path, "fresh", N_CHUNK3)
    big, perm = large(gpu, "normal", N_CHUNK3)
    far = np.random.default_rng(5).integers(0, N_CHUNK3, 100_003, dtype=np.int64)
    small = np.random.default_rng(65).integers(-3, 4, 65).astype(np.float32)
    want_small = argsort_host(gpu, small)
    assert (res["small_0"] == want_small).all() and (res["small_1"] == want_small).all()
    assert same_f64(res["read_0"], f64(big[far])) and same_f64(res["read_1"], f64(big[far]))
    assert (res["large"] == perm).all()
    assert info["bytes"][0] == info["bytes"][1] and info["live"][0] == info["live"][1]
