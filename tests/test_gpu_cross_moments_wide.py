"""Wide cross moments on the device (include/fmhip.h: fmhip_cross_moments_wide) through the C-ABI: Σ x_i·x_j and Σ x_i·y_m of up to 64 vectors
in one launch on the matrix cores (v_mfma_f64_16x16x4_f64).  Every fp32 product is exact in fp64, so the oracle is math.fsum of the exact
products; on small integers every summation order gives the same double, so every entry is exact — which a row/column swap or the f32
forms' result-row formula cannot pass.  The tree of one pair depends on n alone (csrc/xmom_wide_kernel.h), so the bits of a sum do not
depend on the call it was asked for in.  No test here asks the device for anything out of range."""
import ctypes as C
import math
import os
from importlib import import_module

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# mirrors of csrc/xmom_wide_kernel.h
CHUNK, WAVES, TILE, MAX_GRID = 64, 8, 512, 256


def blocks(n):
    return min(max((n + 2 * TILE - 1) // (2 * TILE), 1), MAX_GRID)


def chain(n):
    """L(n), xmom_wide_chain: 64 additions per chunk of a wave, 7 for the waves, grid − 1 for the workgroups."""
    grid = blocks(n)
    chunks = (n + CHUNK - 1) // CHUNK
    return CHUNK * ((chunks + grid * WAVES - 1) // (grid * WAVES)) + (WAVES - 1) + (grid - 1)


def exact(a, b):
    return math.fsum((np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).tolist())


def bound(a, b):
    return 1e-13 * float(np.abs(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)).sum())


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def raw(gpu, hx, n_x, hy, n_y, out=True):
    """fmhip_cross_moments_wide as it stands in the header: (status, buffer)."""
    ax = (C.c_int64 * max(len(hx), 1))(*hx) if hx is not None else None
    ay = (C.c_int64 * max(len(hy), 1))(*hy) if hy is not None else None
    buf = (C.c_double * (64 * 65 // 2 + 64 * 64))()
    return gpu._native.lib().fmhip_cross_moments_wide(ax, n_x, ay, n_y, buf if out else None), buf


def wide(gpu, xs, ys=()):
    """(S, T) of fmhip_cross_moments_wide whatever the counts (regression.cross_moments sends small calls to the narrow pass); None = the constant 1."""
    hx = [0 if v is None else v.handle for v in xs]
    hy = [v.handle for v in ys]
    rc, buf = raw(gpu, hx, len(hx), hy if hy else None, len(hy))
    assert rc == 0, rc
    nx, ny = len(hx), len(hy)
    flat = np.array(buf[: nx * (nx + 1) // 2 + nx * ny])
    S = np.empty((nx, nx))
    iu = np.triu_indices(nx)
    S[iu] = flat[: iu[0].size]
    S.T[iu] = flat[: iu[0].size]
    return S, flat[iu[0].size:].reshape(nx, ny)


SHAPES = [(1, 0), (15, 1), (16, 1), (17, 0), (31, 2), (33, 0), (48, 16), (60, 4), (64, 0), (1, 63)]
# 1 … 65: around a lane's four paths, a round's 16 and a wave's chunk of 64; 511 … 513: the workgroup's 512 paths; 1023 … 1025: where the grid
# takes a second workgroup; 2 x 262144 + 77: past 256 x 1024, where the grid stops growing
SIZES = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2 * 262144 + 77]


@pytest.mark.parametrize("n", SIZES)
def test_exact_on_small_integers(gpu, n):
    """Distinct random vectors of integers in −8 … 8: every partial sum is an integer below 2^53."""
    assert blocks(SIZES[-1]) == MAX_GRID == blocks(SIZES[-1] // 2) and SIZES[-1] <= 1 << 21
    rng = np.random.default_rng(1000 + n)
    pool = rng.integers(-8, 9, (64, n)).astype(np.float32)
    v = [gpu.DeviceVector.from_host(row) for row in pool]
    for n_x, n_y in SHAPES:
        for ones_at in (None, n_x // 2):
            if ones_at is not None and n_x == 1:            # the constant 1 alone among x has no size: the documented error, no launch
                assert raw(gpu, [0], 1, [t.handle for t in v[1:1 + n_y]] or None, n_y)[0] == gpu._native.ERR_INVALID_ARGUMENT
                continue
            cols = pool[: n_x + n_y].astype(np.float64)
            xs = list(v[:n_x])
            if ones_at is not None:
                xs[ones_at] = None
                cols[ones_at] = 1.0
            S, T = wide(gpu, xs, v[n_x:n_x + n_y])
            gram = cols @ cols.T                                            # integers below 2^53: exact in any order
            assert (S == gram[:n_x, :n_x]).all(), (n_x, n_y, ones_at, np.argwhere(S != gram[:n_x, :n_x])[:4])
            assert (T == gram[:n_x, n_x:]).all(), (n_x, n_y, ones_at, np.argwhere(T != gram[:n_x, n_x:])[:4])
            if ones_at is not None: assert S[ones_at, ones_at] == n


def shapes(n, rng):
    yield "normal", rng.standard_normal(n).astype(np.float32)
    yield "lognormal", np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    yield "payoff", np.maximum(rng.standard_normal(n) - 0.2, 0.0).astype(np.float32)
    yield "constant", np.full(n, np.float32(1.25 + 0.125 * rng.integers(0, 8)), dtype=np.float32)
    yield "denormal", (rng.integers(-40, 40, n) * np.float32(1e-45)).astype(np.float32)


@pytest.mark.parametrize("n", [1000, 262_147])
def test_random_data_against_fsum(gpu, n):
    """40 vectors, eight of each shape, as 36 x and 4 y.  1e-13·Σ|a·b| is rigorous for this tree while (L(n) + 1)·2^-53 <= 1e-13."""
    assert (chain(n) + 1) * 2.0 ** -53 <= 1e-13 and chain(n) <= 900
    rng = np.random.default_rng(7 * n)
    data = [a for _ in range(8) for _, a in shapes(n, rng)]
    v = [gpu.DeviceVector.from_host(a) for a in data]
    S, T = wide(gpu, v[:36], v[36:])
    for i in range(36):
        for j in range(i, 36):
            assert abs(S[i, j] - exact(data[i], data[j])) <= bound(data[i], data[j]), (i, j)
        for m in range(4):
            assert abs(T[i, m] - exact(data[i], data[36 + m])) <= bound(data[i], data[36 + m]), (i, m)


def test_bits_do_not_depend_on_the_call(gpu):
    rng = np.random.default_rng(5)
    n = 300_007
    data = [np.exp(0.4 * rng.standard_normal(n)).astype(np.float32) for _ in range(64)]
    v = [gpu.DeviceVector.from_host(a) for a in data]
    a, b = v[3], v[42]
    ref = wide(gpu, [a, b])[0]
    want = (bits(ref[0, 1]), bits(ref[0, 0]), bits(ref[1, 1]))

    def same(S, i, j):
        return (bits(S[min(i, j), max(i, j)]), bits(S[i, i]), bits(S[j, j])) == want

    S64 = wide(gpu, v)[0]
    assert same(S64, 3, 42)                                                     # different groups of 16
    order = list(range(64)); order[4], order[42] = order[42], order[4]
    assert same(wide(gpu, [v[k] for k in order])[0], 3, 4)                      # the same group
    S, T = wide(gpu, v[:40], v[40:])                                            # across the x/y boundary
    assert bits(T[3, 2]) == want[0] and bits(S[3, 3]) == want[1]
    assert bits(wide(gpu, [b, a])[0][0, 1]) == want[0]                          # operands swapped
    assert bits(wide(gpu, [a], [b])[1][0, 0]) == want[0]                        # as T
    assert bits(wide(gpu, [b], [a])[1][0, 0]) == want[0]
    perm = rng.permutation(64)
    Sp = wide(gpu, [v[k] for k in perm])[0]
    assert (bits(Sp) == bits(S64[np.ix_(perm, perm)])).all()                    # the whole list permuted
    # stored, pending, a row of a batched launch; eager and fused; JIT on and off
    twice = wide(gpu, [gpu.DeviceVector.from_host(data[0] * np.float32(2.0)), gpu.DeviceVector.from_host(data[1] * np.float32(2.0))])[0]
    for fusion in (False, True):
        for jit in (gpu.JIT_OFF, gpu.JIT_SYNC):
            prev, prev_jit = gpu.set_fusion(fusion), gpu.set_jit(jit)
            try:
                p0, p1 = v[0].v1s1("MULT_S", 2.0), v[1].v1s1("MULT_S", 2.0)
                got = wide(gpu, [p0, p1])[0]
            finally:
                gpu.set_fusion(prev); gpu.set_jit(prev_jit)
            assert (bits(got) == bits(twice)).all(), (fusion, jit)


def test_nan_and_inf_poison_only_their_entries(gpu):
    rng = np.random.default_rng(11)
    n = 5000
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(20)]
    data[17][1234] = np.nan                                                     # second group of 16
    data[1][77] = np.inf; data[18][77] = 0.0                                    # inf·0 across the two groups
    v = [gpu.DeviceVector.from_host(a) for a in data]
    S, T = wide(gpu, [None] + v[:18], v[18:])
    full = np.hstack([S, T])                                                    # list index: 0 = ones, k + 1 = data[k]
    for i in range(19):
        for j in range(21):
            want_nan = 18 in (i, j) or {i, j} == {2, 19}
            assert np.isnan(full[i, j]) == want_nan, (i, j)
    assert S[2, 2] == np.inf and S[0, 2] == np.inf


def test_argument_errors_launch_nothing(gpu):
    N = gpu._native
    a = gpu.DeviceVector.from_host(np.ones(100, dtype=np.float32))
    b = gpu.DeviceVector.from_host(np.ones(101, dtype=np.float32))
    empty = gpu.DeviceVector.from_host(np.zeros(0, dtype=np.float32))
    prev = gpu.set_fusion(True)
    try:
        pending = a.v1s1("MULT_S", 3.0)
        s0 = gpu.pool_stats()
        h = a.handle
        call = lambda *args, **kw: raw(gpu, *args, **kw)[0]
        assert call([], 0, [h], 1) == N.ERR_INVALID_ARGUMENT
        assert call([h] * 65, 65, [], 0) == N.ERR_INVALID_ARGUMENT
        assert call([h] * 61, 61, [h] * 4, 4) == N.ERR_INVALID_ARGUMENT
        assert call([h], 1, [h] * 64, 64) == N.ERR_INVALID_ARGUMENT
        assert call([h], 1, [], -1) == N.ERR_INVALID_ARGUMENT
        assert call(None, 1, [h], 1) == N.ERR_INVALID_ARGUMENT
        assert call([h], 1, None, 1) == N.ERR_INVALID_ARGUMENT
        assert call([h], 1, [h], 1, out=False) == N.ERR_INVALID_ARGUMENT
        assert call([h] * 20, 20, [0], 1) == N.ERR_INVALID_ARGUMENT                       # the constant 1 is not a y
        assert call([0, 0], 2, [], 0) == N.ERR_INVALID_ARGUMENT                           # nothing has a size
        assert call([h] * 20 + [pending.handle, b.handle], 22, [], 0) == N.ERR_SIZE_MISMATCH
        assert call([pending.handle], 1, [b.handle], 1) == N.ERR_SIZE_MISMATCH
        assert call([h] * 20 + [0x7FFFFFF0], 21, [], 0) == N.ERR_INVALID_HANDLE
        assert empty.n == 0 and call([empty.handle], 1, [], 0) == N.ERR_INVALID_ARGUMENT
        s1 = gpu.pool_stats()
        assert s1.n_kernel_launches == s0.n_kernel_launches and s1.n_ops_executed == s0.n_ops_executed      # the pending operand stays pending
    finally:
        gpu.set_fusion(prev)


def test_one_launch_and_each_pending_vector_computed_once(gpu):
    rng = np.random.default_rng(13)
    n = 50_000
    base = [gpu.DeviceVector.from_host(rng.standard_normal(n).astype(np.float32)) for _ in range(40)]
    before = gpu.pool_stats().n_kernel_launches
    wide(gpu, base[:36], base[36:])
    assert gpu.pool_stats().n_kernel_launches - before == 1
    prev = gpu.set_fusion(True)
    try:
        pend = [b.v1s1("MULT_S", 1.5) for b in base]
        s0 = gpu.pool_stats()
        S, T = wide(gpu, pend[:36], pend[36:])
        s1 = gpu.pool_stats()
        assert s1.n_ops_executed - s0.n_ops_executed == 40                 # every pending vector once
        assert s1.n_kernel_launches - s0.n_kernel_launches - 1 >= 1         # the flush, then the pass
        S2, T2 = wide(gpu, pend[:36], pend[36:])                           # stored now: the pass alone
        assert gpu.pool_stats().n_kernel_launches - s1.n_kernel_launches == 1
        assert gpu.pool_stats().n_ops_executed == s1.n_ops_executed
        assert (bits(S) == bits(S2)).all() and (bits(T) == bits(T2)).all()
    finally:
        gpu.set_fusion(prev)


class wide_knob_off:
    def __enter__(self):
        self.prev = os.environ.get("FMHIP_DEVICE_WIDE_MOMENTS")
        os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = "0"
    def __exit__(self, *a):
        if self.prev is None: del os.environ["FMHIP_DEVICE_WIDE_MOMENTS"]
        else: os.environ["FMHIP_DEVICE_WIDE_MOMENTS"] = self.prev


def test_estimator_takes_the_one_pass_path_at_twenty_regressors(gpu):
    """K = 20 independent standard normals plus the constant: A = XᵀX/n is I + O(n^-1/2) (every off-diagonal entry within ~4.5/sqrt(n) ≈ 0.015,
    so by Gershgorin κ(A) <= (1 + 21·0.015)/(1 − 21·0.015) < 2 — asserted below).  The sums are within 1e-13·Σ|a·b| of the exact ones, so
    the coefficients are within about κ·K·1e-13 of those of the exact sums: 1e-9 is that with a wide margin."""
    n, K = 100_000, 20
    rng = np.random.default_rng(17)
    X = rng.standard_normal((K, n)).astype(np.float32)
    coef = rng.uniform(-1.0, 1.0, K + 1)
    y = (coef[0] + coef[1:] @ X.astype(np.float64) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    f = gpu.RandomVariableHipFactory()
    basis = [f.createRandomVariable(1.0)] + [f.createRandomVariable(0.0, x) for x in X]
    dep = f.createRandomVariable(0.0, y)
    est = gpu.MonteCarloConditionalExpectationRegression(basis)
    before = gpu.pool_stats().n_kernel_launches
    beta = est.getLinearRegressionParameters(dep)
    assert gpu.pool_stats().n_kernel_launches - before == 1                 # everything is stored: no flush, one pass
    cols = [np.ones(n, dtype=np.float32)] + list(X)
    A = np.array([[exact(cols[i], cols[j]) for j in range(K + 1)] for i in range(K + 1)]) / n
    b = np.array([exact(c, y) for c in cols]) / n
    assert np.linalg.cond(A) <= 2.0
    A_dev, b_dev = est._normal_equations_device([dep])
    for i in range(K + 1):
        for j in range(K + 1):
            assert abs(A_dev[i, j] - A[i, j]) * n <= bound(cols[i], cols[j]), (i, j)
        assert abs(b_dev[i, 0] - b[i]) * n <= bound(cols[i], y), i
    assert np.abs(beta - gpu.solve_normal_equations(A, b)).max() <= 1e-9
    with wide_knob_off():
        before = gpu.pool_stats().n_kernel_launches
        generic = est.getLinearRegressionParameters(dep)
        assert gpu.pool_stats().n_kernel_launches - before > 100           # pair by pair: K(K+3)/2 products and averages
    assert np.abs(generic - beta).max() <= 1e-4                             # fp32 products: the same fit to their rounding


def test_max_call_driver(gpu, monkeypatch):
    """2 assets, all monomials up to degree 3 — 10 basis functions, the constant among them —, 2^16 paths, 9 exercise dates: one regression,
    ONE launch, per exercise date at which there is a continuation value to estimate (all but the last).  Ten functions are within the
    narrow pass's 12, so the same is asked at degree 5 — 21 functions, the wide pass — as well."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    reg = import_module("finmath-lib-cuda-extensions_amd.regression")
    dates = [3.0 * k / 9 for k in range(1, 10)]
    bm = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 9, 3.0 / 9), 2, 1 << 16, 4711)
    run = lambda ds, order: mc.bermudan_max_call_mc(bm, [100.0, 100.0], 0.05, 0.10, 0.20, ds, 100.0, basis_order=order)
    calls = []
    inner = reg.cross_moments

    def counted(xs, ys=()):
        before = gpu.pool_stats().n_kernel_launches
        out = inner(xs, ys)
        calls.append((len(list(xs)), gpu.pool_stats().n_kernel_launches - before))
        return out

    monkeypatch.setattr(reg, "cross_moments", counted)
    prev = gpu.set_fusion(False)                                              # eager: nothing is pending when the pass is asked for
    try:
        for order, functions in ((3, 10), (5, 21)):
            assert len(mc.monomial_exponents(2, order)) == functions
            del calls[:]
            value, error = run(dates, order)
            assert calls == [(functions, 1)] * (len(dates) - 1), calls
            with wide_knob_off():
                generic, _ = run(dates, order)                                # beyond 12 functions: pair by pair, on the same paths
            european, _ = run(dates[-1:], order)
            print(f"max-call, 2 assets, degree {order}, 65536 paths: {value:.4f} ± {error:.4f}; knob off {generic:.4f}; European {european:.4f}")
            assert abs(value - generic) <= 3.0 * error
            assert value > european
    finally:
        gpu.set_fusion(prev)


def test_communicator_answers_for_the_global_sample(gpu):
    rng = np.random.default_rng(21)
    n, m = 40_000, 20
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(m)]
    halves = [[gpu.DeviceVector.from_host(a[: n // 2]) for a in data], [gpu.DeviceVector.from_host(a[n // 2:]) for a in data]]
    ask = lambda h: wide(gpu, [None] + h[:-1], [h[-1]])
    flat = lambda S, T: np.concatenate([S[np.triu_indices(m)], T.ravel()])
    local = [ask(h) for h in halves]
    try:
        for rank in (0, 1):
            calls = []

            def gather(mine, rank=rank):
                calls.append(mine.copy())
                theirs = flat(*local[1 - rank])
                return np.stack([mine, theirs] if rank == 0 else [theirs, mine])

            gpu.set_expectation_comm(2, rank, gather)
            S, T = ask(halves[rank])
            assert len(calls) == 1 and (bits(calls[0]) == bits(flat(*local[rank]))).all()              # one gather, of the local sums
            assert S[0, 0] == n
            assert (bits(flat(S, T)) == bits(flat(*local[0]) + flat(*local[1]))).all()                # added in rank order
    finally:
        gpu.set_expectation_comm(1, 0, None)


_DEVICES = r'''
import ctypes as C, importlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
rng = np.random.default_rng(31)
n, m = 100_003, 20
data = [rng.standard_normal(n).astype(np.float32) for _ in range(m)]

def ask(vs):
    hx = (C.c_int64 * m)(0, *[v.handle for v in vs[:-1]])
    hy = (C.c_int64 * 1)(vs[-1].handle)
    out = (C.c_double * (m * (m + 1) // 2 + m))()
    rc = fm._native.lib().fmhip_cross_moments_wide(hx, m, hy, 1, out)
    assert rc == 0, rc
    return list(out)

fm.init_devices([0, 0])
fm.set_fusion(True)
x = [fm.DeviceVector.from_host(a) for a in data]
out = {"stored": ask(x), "pending": ask([v.v1s1("MULT_S", 2.0) for v in x])}
out["tiny"] = ask([fm.DeviceVector.from_host(a[:1]) for a in data])      # a vector shorter than the shards are many
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


def test_device_list(tmp_path):
    """A device list {0, 0}: every shard runs the pass on its block of paths, the front adds the sums in shard order — the sums of the whole
    sample within the reassociation bound, n exactly.  In a process of its own."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "devices.py"
    script.write_text(_DEVICES % {"root": root})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    rng = np.random.default_rng(31)
    n, m = 100_003, 20
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(m)]
    for key, scale, size in (("stored", 1.0, n), ("pending", 2.0, n), ("tiny", 1.0, 1)):
        cols = [np.ones(size, dtype=np.float32)] + [a[:size] * np.float32(scale) for a in data]
        flat = out[key]
        assert flat[0] == size, key
        at = 0
        for i in range(m):
            for j in range(i, m):
                assert abs(flat[at] - exact(cols[i], cols[j])) <= bound(cols[i], cols[j]), (key, i, j)
                at += 1
        for i in range(m):
            assert abs(flat[at + i] - exact(cols[i], cols[m])) <= bound(cols[i], cols[m]), (key, i)
