"""Sort on the device (include/fmhip.h: fmhip_sort_by_key, fmhip_argsort, fmhip_rank_scores, fmhip_vec_read_elements)
through the C-ABI and the Python mirror.  A stable sort has one right answer: every check is an equality with the host definition
(fmhip_argsort_host, itself checked against numpy's stable argsort of the keys in tests/test_sort_cpu.py) or with numpy.  Sizes come from
the constants of csrc/sort_host.hpp, read from the header.  No test here asks the device for anything out of range: bad arguments are
refused on the host before a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_sort_cpu import argsort_host, inputs, keys

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
