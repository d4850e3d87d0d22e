"""Cross moments on the device (include/fmhip.h: fmhip_cross_moments) through the C-ABI: Σ x_i·x_j and Σ x_i·y_m of up to 12 + 4 vectors in
one launch.  Every fp32 product is exact in fp64, so the oracle is math.fsum of the exact products; the order of the additions of one pair
depends on n alone, so the bits of a sum do not depend on the call it was asked for in.  No test here asks the device for anything out of
range: bad arguments are refused on the host before a launch."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def exact(a, b):
    return math.fsum((np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).tolist())


def bound(a, b):
    return 1e-13 * float(np.abs(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).sum())


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 2047, 2048, 2049, 100_001, 1 << 20, (1 << 24) + 3])
def test_exact_on_small_integers(gpu, n):
    rng = np.random.default_rng(n)
    cols = [rng.integers(-8, 9, n).astype(np.float32) for _ in range(3)]
    dep = rng.integers(-8, 9, n).astype(np.float32)
    v = [gpu.DeviceVector.from_host(c) for c in cols]
    S, T = gpu.cross_moments([None] + v, [gpu.DeviceVector.from_host(dep)])
    full = [np.ones(n)] + [c.astype(np.float64) for c in cols]
    for i in range(4):
        for j in range(4):
            assert S[i, j] == float(np.dot(full[i].astype(np.int64), full[j].astype(np.int64))), (i, j)
        assert T[i, 0] == float(np.dot(full[i].astype(np.int64), dep.astype(np.int64)))
    assert S[0, 0] == n


def shapes(n, rng):
    yield "normal", rng.standard_normal(n).astype(np.float32)
    yield "lognormal", np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    yield "payoff", np.maximum(rng.standard_normal(n) - 0.2, 0.0).astype(np.float32)
    yield "constant", np.full(n, 1.25, dtype=np.float32)
    yield "denormal", (rng.integers(-40, 40, n) * np.float32(1e-45)).astype(np.float32)


@pytest.mark.parametrize("n", [1000, 262_147])
def test_random_data_against_fsum(gpu, n):
    rng = np.random.default_rng(7 * n)
    data = [a for _, a in shapes(n, rng)]
    v = [gpu.DeviceVector.from_host(a) for a in data]
    S, T = gpu.cross_moments(v, v[:2])
    for i in range(5):
        for j in range(5):
            assert abs(S[i, j] - exact(data[i], data[j])) <= bound(data[i], data[j]), (i, j)
        for m in range(2):
            assert abs(T[i, m] - exact(data[i], data[m])) <= bound(data[i], data[m]), (i, m)
            assert bits(T[i, m]) == bits(S[i, m])                      # the same pair as T and as S


def test_bits_do_not_depend_on_the_call(gpu):
    rng = np.random.default_rng(5)
    n = 300_007
    data = [np.exp(0.4 * rng.standard_normal(n)).astype(np.float32) for _ in range(12)]
    ys = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    v = [gpu.DeviceVector.from_host(a) for a in data]
    w = [gpu.DeviceVector.from_host(a) for a in ys]
    a, b = v[3], v[10]
    ref = gpu.cross_moments([a, b])[0]
    S12, T12 = gpu.cross_moments(v, w)
    assert bits(S12[3, 10]) == bits(ref[0, 1]) and bits(S12[3, 3]) == bits(ref[0, 0]) and bits(S12[10, 10]) == bits(ref[1, 1])
    assert bits(gpu.cross_moments([b, a])[0][0, 1]) == bits(ref[0, 1])                       # operands swapped
    assert bits(gpu.cross_moments([a], [b])[1][0, 0]) == bits(ref[0, 1])                     # as T
    perm = rng.permutation(12)
    Sp, Tp = gpu.cross_moments([v[k] for k in perm], w[::-1])
    assert (bits(Sp) == bits(S12[np.ix_(perm, perm)])).all()                                 # the list permuted
    assert (bits(Tp) == bits(T12[perm][:, ::-1])).all()
    # a dependent in the first group of eight and in the second: the same pair from two different blocks of the launch
    assert bits(gpu.cross_moments(v[:3], [w[0]])[1][1, 0]) == bits(T12[1, 0])
    # stored, pending, a row of a batched launch; eager and fused; JIT on and off
    want = gpu.cross_moments([gpu.DeviceVector.from_host(data[0] * np.float32(2.0)), gpu.DeviceVector.from_host(data[1] * np.float32(2.0))])[0]
    for fusion in (False, True):
        for jit in (gpu.JIT_OFF, gpu.JIT_SYNC):
            prev, prev_jit = gpu.set_fusion(fusion), gpu.set_jit(jit)
            try:
                p0, p1 = v[0].v1s1("MULT_S", 2.0), v[1].v1s1("MULT_S", 2.0)               # pending when fused: one batched launch of two rows
                got = gpu.cross_moments([p0, p1])[0]
            finally:
                gpu.set_fusion(prev); gpu.set_jit(prev_jit)
            assert (bits(got) == bits(want)).all(), (fusion, jit)


def test_ones_entry(gpu):
    rng = np.random.default_rng(9)
    n = 123_457
    data = [rng.standard_normal(n).astype(np.float32) + np.float32(0.5) for _ in range(3)]
    v = [gpu.DeviceVector.from_host(a) for a in data]
    S, T = gpu.cross_moments([1.0] + v + [None], [v[0]])
    assert S[0, 0] == n and S[0, 4] == n and S[4, 4] == n
    for j in range(3):
        assert abs(S[0, j + 1] - v[j].moments().sum) <= 1e-13 * float(np.abs(data[j]).astype(np.float64).sum())
        assert bits(S[4, j + 1]) == bits(S[0, j + 1])
    assert abs(T[0, 0] - v[0].moments().sum) <= 1e-13 * float(np.abs(data[0]).astype(np.float64).sum())
    C_ = gpu.covariance_matrix(v)
    assert np.allclose(C_, np.cov(np.stack(data).astype(np.float64), bias=True), rtol=0, atol=1e-12)


def test_nan_and_inf_poison_only_their_entries(gpu):
    rng = np.random.default_rng(11)
    n = 5000
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(5)]
    data[3][1234] = np.nan
    data[1][77] = np.inf; data[2][77] = 0.0
    v = [gpu.DeviceVector.from_host(a) for a in data]
    S, T = gpu.cross_moments([None] + v, [v[4]])
    for i in range(6):
        for j in range(6):
            want_nan = 4 in (i, j) or {i, j} == {2, 3}                 # x_3 is entry 4 of the list with the ones; inf·0 between entries 2 and 3
            assert np.isnan(S[i, j]) == want_nan, (i, j)
    assert S[2, 2] == np.inf and S[0, 2] == np.inf
    assert [bool(np.isnan(t)) for t in T[:, 0]] == [False, False, False, False, True, False]


def _call(fm, x, n_x, y, n_y, out=True):
    hx = (C.c_int64 * max(len(x), 1))(*x) if x is not None else None
    hy = (C.c_int64 * max(len(y), 1))(*y) if y is not None else None
    buf = (C.c_double * 256)()
    return fm.lib().fmhip_cross_moments(hx, n_x, hy, n_y, buf if out else None)


def test_argument_errors_launch_nothing(gpu):
    N = gpu._native
    a = gpu.DeviceVector.from_host(np.ones(100, dtype=np.float32))
    b = gpu.DeviceVector.from_host(np.ones(101, dtype=np.float32))
    empty = gpu.DeviceVector.from_host(np.zeros(0, dtype=np.float32)) if hasattr(gpu.DeviceVector, "from_host") else None
    prev = gpu.set_fusion(True)
    try:
        pending = a.v1s1("MULT_S", 3.0)
        before = gpu.pool_stats().n_kernel_launches
        h = a.handle
        assert _call(gpu, [h] * 13, 13, [], 0) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [], 0, [h], 1) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [h], 1, [h] * 5, 5) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [h], 1, [], -1) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, None, 1, [h], 1) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [h], 1, None, 1) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [h], 1, [h], 1, out=False) == N.ERR_INVALID_ARGUMENT
        assert _call(gpu, [h], 1, [0], 1) == N.ERR_INVALID_ARGUMENT                       # the constant 1 is not a y
        assert _call(gpu, [0, 0], 2, [], 0) == N.ERR_INVALID_ARGUMENT                     # nothing has a size
        assert _call(gpu, [h, pending.handle, b.handle], 3, [], 0) == N.ERR_SIZE_MISMATCH
        assert _call(gpu, [pending.handle], 1, [b.handle], 1) == N.ERR_SIZE_MISMATCH
        assert _call(gpu, [h, 0x7FFFFFF0], 2, [], 0) == N.ERR_INVALID_HANDLE
        if empty is not None and empty.n == 0:
            assert _call(gpu, [empty.handle], 1, [], 0) == N.ERR_INVALID_ARGUMENT
        assert gpu.pool_stats().n_kernel_launches == before                               # not even the pending operand was computed
    finally:
        gpu.set_fusion(prev)


def test_given_up_values_are_the_documented_error(gpu):
    """Where the engine did not store a value that was given up, its cross moments are the error a read is; where it kept it, the right answer."""
    prev = gpu.set_fusion(True)
    try:
        x = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
        ys = [x.v1s1("ADD_S", float(k)) for k in range(1, 5)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for k, y in enumerate(ys, start=1):
            try:
                assert gpu.cross_moments([None, y])[0][0, 1] == 4096 * 4095 / 2 + 4096 * k
            except gpu.FmhipError as e:
                assert e.code == gpu._native.ERR_INVALID_ARGUMENT and "given up" in str(e)
    finally:
        gpu.set_fusion(prev)


def test_one_launch_and_each_pending_vector_computed_once(gpu):
    rng = np.random.default_rng(13)
    n = 50_000
    base = [gpu.DeviceVector.from_host(rng.standard_normal(n).astype(np.float32)) for _ in range(16)]
    before = gpu.pool_stats().n_kernel_launches
    gpu.cross_moments(base[:12], base[12:])
    assert gpu.pool_stats().n_kernel_launches - before == 1
    prev = gpu.set_fusion(True)
    try:
        pend = [b.v1s1("MULT_S", 1.5) for b in base]
        s0 = gpu.pool_stats()
        S, T = gpu.cross_moments(pend[:12] + [], pend[12:])
        s1 = gpu.pool_stats()
        assert s1.n_ops_executed - s0.n_ops_executed == 16                 # every pending vector once
        flush = s1.n_kernel_launches - s0.n_kernel_launches - 1
        S2, T2 = gpu.cross_moments(pend[:12], pend[12:])                   # stored now: the pass alone
        assert gpu.pool_stats().n_kernel_launches - s1.n_kernel_launches == 1 and flush >= 1
        assert gpu.pool_stats().n_ops_executed == s1.n_ops_executed
        assert (bits(S) == bits(S2)).all() and (bits(T) == bits(T2)).all()
    finally:
        gpu.set_fusion(prev)


def test_communicator_answers_for_the_global_sample(gpu):
    rng = np.random.default_rng(21)
    n = 40_000
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    whole = [gpu.DeviceVector.from_host(a) for a in data]
    halves = [[gpu.DeviceVector.from_host(a[: n // 2]) for a in data], [gpu.DeviceVector.from_host(a[n // 2:]) for a in data]]
    want_S, want_T = gpu.cross_moments([None] + whole[:2], [whole[2]])
    local = [gpu.cross_moments([None] + h[:2], [h[2]]) for h in halves]
    flat = lambda S, T: np.concatenate([S[np.triu_indices(3)], T.ravel()])
    try:
        for rank in (0, 1):
            calls = []

            def gather(mine, rank=rank):
                calls.append(mine.copy())
                theirs = flat(*local[1 - rank])
                return np.stack([mine, theirs] if rank == 0 else [theirs, mine])

            gpu.set_expectation_comm(2, rank, gather)
            S, T = gpu.cross_moments([None] + halves[rank][:2], [halves[rank][2]])
            assert len(calls) == 1 and (bits(calls[0]) == bits(flat(*local[rank]))).all()              # one gather, of the local sums
            assert S[0, 0] == n
            assert (np.abs(S - want_S) <= 1e-13 * n * 25).all() and (np.abs(T - want_T) <= 1e-13 * n * 25).all()
            assert (bits(flat(S, T)) == bits(flat(*local[0]) + flat(*local[1]))).all()                # added in rank order
    finally:
        gpu.set_expectation_comm(1, 0, None)


_OTHER_MODES = r'''
import importlib, json, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode = sys.argv[1]
rng = np.random.default_rng(31)
n = 100_003
data = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]

def ask(vs):
    S, T = fm.cross_moments([None] + vs[:2], [vs[2]])
    return {"S": S.tolist(), "T": T.tolist()}

if mode == "devices":
    fm.init_devices([0, 0])
    fm.set_fusion(True)
    x = [fm.DeviceVector.from_host(a) for a in data]
    out = {"stored": ask(x), "pending": ask([v.v1s1("MULT_S", 2.0) for v in x])}
    tiny = [fm.DeviceVector.from_host(a[:1]) for a in data]      # a vector shorter than the shards are many
    out["tiny"] = ask(tiny)
else:
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    x = [fm.DeviceVector.from_host(a) for a in data]
    y = [v.v1s1("MULT_S", 2.0) for v in x]                       # pending, owned by the main thread's engine
    out = {}
    def other():
        out["stored"] = ask(x); out["pending"] = ask(y)
    t = threading.Thread(target=other); t.start(); t.join()
    out["tiny"] = ask([fm.DeviceVector.from_host(a[:1]) for a in data])
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(mode, tmp_path):
    """A device list {0, 0} (every shard runs the pass on its block of paths, the front adds the sums in shard order) and vectors of another
    thread's engine: the sums of the whole sample within the reassociation bound, n exactly.  In a process of its own."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": root})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    rng = np.random.default_rng(31)
    n = 100_003
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(3)]
    for key, scale, m in (("stored", 1.0, n), ("pending", 2.0, n), ("tiny", 1.0, 1)):
        cols = [np.ones(m, dtype=np.float32)] + [a[:m] * np.float32(scale) for a in data]
        S, T = np.array(out[key]["S"]), np.array(out[key]["T"])
        assert S[0, 0] == m, key
        for i in range(3):
            for j in range(3):
                assert abs(S[i, j] - exact(cols[i], cols[j])) <= bound(cols[i], cols[j]), (key, i, j)
            assert abs(T[i, 0] - exact(cols[i], cols[3])) <= bound(cols[i], cols[3]), (key, i)
