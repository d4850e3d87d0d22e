"""Polynomial regression in one pass on the device (include/fmhip.h: fmhip_polynomial_cross_moments, fmhip_polynomial_evaluate; DESIGN.md
§4.15): the sums are fmhip_cross_moments_wide's, bit for bit, for the same list with the monomials materialised by the mirror's mult chain;
exact on small integers; within the tree's bound of math.fsum; NaN / inf stay where their exponents put them; the evaluation is the recorded
mult / addProduct chain bit for bit; the estimator and the max-call driver agree with the materialised path to the last bit; device lists."""
import ctypes as C
import math
import os
from contextlib import contextmanager
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


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _poly_constants():
    """FM_POLY_EVAL_BLOCK and FM_POLY_EVAL_MAX_BLOCKS of csrc/xmom_poly_kernel.h."""
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "finmath-lib-cuda-extensions_amd", "csrc", "xmom_poly_kernel.h")).read()
    return {name: int(value) for name, value in re.findall(r"constexpr int (FM_POLY_EVAL_\w+) = (\d+);", text)}


# the evaluation's grid stops growing at FM_POLY_EVAL_MAX_BLOCKS workgroups of FM_POLY_EVAL_BLOCK lanes, a quad each: 1029 elements more put
# lanes of two workgroups on a second trip of the grid-stride loop, the last of them with a ragged quad
EVAL_TRIP = _poly_constants()["FM_POLY_EVAL_MAX_BLOCKS"] * 4 * _poly_constants()["FM_POLY_EVAL_BLOCK"]
EVAL_SECOND_TRIP = (2, 3, 1, 0, EVAL_TRIP + 1029)              # (n_states, order, n_extra, n_y, n): 4 195 333 with today's constants
assert EVAL_SECOND_TRIP[4] > EVAL_TRIP and EVAL_SECOND_TRIP[4] % 4 != 0 and EVAL_SECOND_TRIP[4] - EVAL_TRIP > 4 * _poly_constants()["FM_POLY_EVAL_BLOCK"]


def reg():
    return import_module("finmath-lib-cuda-extensions_amd.regression")


def exponents_of(n_states, order):
    return import_module("finmath-lib-cuda-extensions_amd.montecarlo").monomial_exponents(n_states, order)


def wide(gpu, xs, ys=()):
    """(S, T) of fmhip_cross_moments_wide, called directly whatever the counts; None = the constant 1."""
    hx = [0 if v is None else v.realizations.handle for v in xs]
    hy = [v.realizations.handle for v in ys]
    nx, ny = len(hx), len(hy)
    buf = (C.c_double * (nx * (nx + 1) // 2 + nx * ny))()
    rc = gpu._native.lib().fmhip_cross_moments_wide((C.c_int64 * nx)(*hx), nx, (C.c_int64 * max(ny, 1))(*hy) if ny else None, ny, buf)
    assert rc == 0, rc
    flat = np.array(buf[:])
    S = np.empty((nx, nx))
    iu = np.triu_indices(nx)
    S[iu] = flat[: iu[0].size]
    S.T[iu] = flat[: iu[0].size]
    return S, flat[iu[0].size:].reshape(nx, ny)


def materialised(gpu, states, exponents):
    """The monomials through the mirror's mult chain; a row of zeros is None (the constant 1, handle 0)."""
    one = gpu.RandomVariableHip(-math.inf, 1.0)
    return [None if f is one else f for f in reg().monomial_basis(states, exponents, one)]


def rvs(gpu, arrays):
    return [gpu.RandomVariableHip(0.0, gpu.DeviceVector.from_host(a)) for a in arrays]


@contextmanager
def knob(value):
    old = os.environ.get("FMHIP_DEVICE_POLYNOMIAL_MOMENTS")
    os.environ["FMHIP_DEVICE_POLYNOMIAL_MOMENTS"] = value
    try: yield
    finally:
        if old is None: del os.environ["FMHIP_DEVICE_POLYNOMIAL_MOMENTS"]
        else: os.environ["FMHIP_DEVICE_POLYNOMIAL_MOMENTS"] = old


# (n_states, order, n_extra, n_y)
FIRST, FOUR_GROUPS = (1, 1, 0, 0), (5, 3, 0, 1)
OTHERS = [(1, 6, 0, 1), (2, 3, 0, 1), (3, 3, 1, 4), (5, 3, 3, 5), (8, 1, 0, 0), (8, 2, 2, 1)]
# 1, 3: the tail inside a 16-byte load; 63 … 65: a chunk's edge; 511, 513: a second chunk per wave; 1024, 1025: a second workgroup; 4099: several;
# 262147: past the cap of 256 workgroups
SIZES = [1, 3, 63, 64, 65, 511, 513, 1024, 1025, 4099, 262_147]
CASES = [(s, n) for n in SIZES for s in (FIRST, FOUR_GROUPS)] + [(s, n) for n in (1025, 4099) for s in OTHERS]


def _data(shape, n, seed):
    ns, order, ne, ny = shape
    rng = np.random.default_rng(seed)
    states = [np.exp(0.25 * rng.standard_normal(n)).astype(np.float32) for _ in range(ns)]
    extra = [np.maximum(rng.standard_normal(n), 0.0).astype(np.float32) for _ in range(ne)]
    ys = [rng.standard_normal(n).astype(np.float32) for _ in range(ny)]
    return states, extra, ys


@pytest.mark.parametrize("shape,n", CASES, ids=[f"{s[0]}s-deg{s[1]}-{s[2]}x-{s[3]}y-n{n}" for s, n in CASES])
def test_bits_are_the_wide_pass_on_the_materialised_monomials(gpu, shape, n):
    assert blocks(262_147) == MAX_GRID
    ns, order, ne, ny = shape
    r = reg()
    a_states, a_extra, a_ys = _data(shape, n, 100 * n + ns + order)
    states, extra, ys = rvs(gpu, a_states), rvs(gpu, a_extra), rvs(gpu, a_ys)
    if ne: extra[0] = None                                                   # the constant 1 among the extra vectors
    table = exponents_of(ns, order)
    assert len(table) + ne + ny <= 64
    rng = np.random.default_rng(n)
    for exps in (table, [table[i] for i in rng.permutation(len(table))]):
        want = wide(gpu, materialised(gpu, states, exps) + extra, ys)
        got = r.polynomial_cross_moments(states, exps, extra, ys)
        assert np.array_equal(bits(got[0]), bits(want[0])), (shape, n, np.argwhere(bits(got[0]) != bits(want[0]))[:4])
        assert np.array_equal(bits(got[1]), bits(want[1])), (shape, n)
    # pending (unflushed) states: the pass computes them in its one flush
    prev = gpu.set_fusion(True)
    try:
        pending = [s.mult(1.0009765625) for s in states]
        got = r.polynomial_cross_moments(pending, table, extra, ys)
    finally:
        gpu.set_fusion(prev)
    stored = rvs(gpu, [(a * np.float32(1.0009765625)).astype(np.float32) for a in a_states])
    want = wide(gpu, materialised(gpu, stored, table) + extra, ys)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (shape, n, "pending")


@pytest.mark.parametrize("n", [65, 1025, 262_147])
def test_exact_on_small_integers(gpu, n):
    """States in −3 … 3, three of them, degree 3: every monomial, product and partial sum is an integer far below 2^53 — the lane maps without
    reference to the wide kernel."""
    rng = np.random.default_rng(2000 + n)
    a = rng.integers(-3, 4, (3, n))
    y = rng.integers(-3, 4, n)
    table = exponents_of(3, 3)
    cols = np.array([np.prod([a[s] ** e[s] for s in range(3)], axis=0) for e in table] + [y], dtype=np.int64)
    S, T = reg().polynomial_cross_moments(rvs(gpu, a.astype(np.float32)), table, (), rvs(gpu, [y.astype(np.float32)]))
    gram = cols @ cols.T
    assert (S == gram[:20, :20]).all() and (T[:, 0] == gram[:20, 20]).all()
    assert S[0, 0] == n


def shapes(n, rng):
    yield "normal", rng.standard_normal(n).astype(np.float32)
    yield "lognormal", np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    yield "payoff", np.maximum(rng.standard_normal(n) - 0.2, 0.0).astype(np.float32)
    yield "constant", np.full(n, np.float32(1.25 + 0.125 * rng.integers(0, 8)), dtype=np.float32)
    yield "denormal", (rng.integers(-40, 40, n) * np.float32(1e-45)).astype(np.float32)


def _f32_monomial(arrays, e):
    t = None
    for s, es in enumerate(e):
        if not es: continue
        p = arrays[s]
        for _ in range(es - 1): p = (p * arrays[s]).astype(np.float32)
        t = p if t is None else (t * p).astype(np.float32)
    return np.ones_like(arrays[0]) if t is None else t


@pytest.mark.parametrize("n", [1000, 262_147])
def test_random_data_against_fsum(gpu, n):
    """Five states, one of each kind of data (denormals among them), degree 2 (21 terms) and the five as dependents: every entry within
    (L(n) + 1)·2^-53·Σ|a·b| of math.fsum over the fp32 monomials."""
    rng = np.random.default_rng(7 * n)
    data = [a for _, a in shapes(n, rng)]
    ys = [a for _, a in shapes(n, rng)]
    table = exponents_of(5, 2)
    cols = [_f32_monomial(data, e).astype(np.float64) for e in table] + [y.astype(np.float64) for y in ys]
    S, T = reg().polynomial_cross_moments(rvs(gpu, data), table, (), rvs(gpu, ys))
    got = np.hstack([S, T])
    u = (chain(n) + 1) * 2.0 ** -53
    for i in range(21):
        for j in range(i, 26):
            prod = cols[i] * cols[j]
            assert abs(got[i, j] - math.fsum(prod.tolist())) <= u * float(np.abs(prod).sum()), (i, j, got[i, j])


def test_nan_and_inf_poison_only_their_entries(gpu):
    n = 1500
    rng = np.random.default_rng(5)
    a = [np.exp(0.2 * rng.standard_normal(n)).astype(np.float32) for _ in range(4)]
    a[2][777] = np.nan
    a[3][1499] = np.inf
    table = [e for e in exponents_of(4, 2) if e[3] == 0]                    # the infinite state takes part nowhere: exponent 0 throughout
    S, T = reg().polynomial_cross_moments(rvs(gpu, a), table, (), rvs(gpu, [a[0]]))
    uses = np.array([e[2] != 0 for e in table])
    assert uses.any() and not uses.all()
    assert np.array_equal(np.isnan(S), uses[:, None] | uses[None, :])
    assert np.array_equal(np.isnan(T[:, 0]), uses)
    assert np.isfinite(S[~uses][:, ~uses]).all()


@pytest.mark.parametrize("shape", [FIRST, FOUR_GROUPS] + OTHERS + [EVAL_SECOND_TRIP], ids=lambda s: "-".join(map(str, s)))
def test_evaluate_is_the_recorded_chain_bit_for_bit(gpu, shape):
    ns, order, ne, _ = shape[:4]
    r = reg()
    table = exponents_of(ns, order)
    K = len(table) + ne
    if K > 60: table = table[: 60 - ne]; K = 60
    # (n, the first extra vector is the constant 1); a shape that names a size is evaluated at that size, with the extra vector and with the constant
    cases = [(shape[4], False), (shape[4], True)] if len(shape) > 4 else [(n, False) for n in (1, 3, 5, 1023, 1025, 4099)]
    for n, constant in cases:
        a_states, a_extra, _ = _data(shape[:4], n, 31 * n + K)
        states, extra = rvs(gpu, a_states), rvs(gpu, a_extra)
        beta = np.random.default_rng(n + K).standard_normal(K)
        one = gpu.RandomVariableHip(-math.inf, 1.0)
        if constant: extra[0] = one
        basis = r.monomial_basis(states, table, one) + extra
        ce = basis[0].mult(float(beta[0]))
        for i in range(1, K): ce = ce.addProduct(basis[i], float(beta[i]))
        want = ce.getRealizations() if not ce.isDeterministic() else np.full(n, ce.doubleValue())
        out = gpu.RandomVariableHip(0.0, r.polynomial_evaluate(states, table, beta, [None] + extra[1:] if constant else extra))
        got = out.getRealizations()
        assert got.shape == (n,)
        assert np.array_equal(got.astype(np.float32).view(np.uint32), np.asarray(want, dtype=np.float32).view(np.uint32)), (shape, n)
        if not ce.isDeterministic():
            assert out.add(1.0).sub(1.0).size() == n                            # a vector that further methods accept
            assert out.getAverage() == ce.getAverage()


def test_estimator_is_the_materialised_estimator_bit_for_bit(gpu):
    r = reg()
    n = 20_011
    a_states, a_extra, a_ys = _data((3, 3, 1, 5), n, 77)
    states, extra, ys = rvs(gpu, a_states), rvs(gpu, a_extra), rvs(gpu, a_ys)
    est = r.MonteCarloConditionalExpectationPolynomialRegression(states, order=3, extra_basis=extra)       # K = 21 > 12: the wide pass with the knob off
    assert est._one_pass(ys)
    beta_on = est.getLinearRegressionParameters(ys)
    ce_on = [c.getRealizations() for c in est.getConditionalExpectation(ys)]
    with knob("0"):
        assert not est._one_pass(ys)
        beta_off = est.getLinearRegressionParameters(ys)
        ce_off = [c.getRealizations() for c in est.getConditionalExpectation(ys)]
    assert beta_on.shape == (21, 5) and np.array_equal(bits(beta_on), bits(beta_off))
    for a, b in zip(ce_on, ce_off): assert np.array_equal(bits(a), bits(b))
    one_on = est.getConditionalExpectation(ys[0]).getRealizations()
    assert np.array_equal(bits(one_on), bits(ce_on[0]))


def test_max_call_driver_one_pass_basis(gpu):
    """3 assets, degree 3 (20 functions: the default takes the wide pass), 4 dates, 16 384 paths: the same value to the last bit, in fewer
    launches per date — no monomial is built, no chain is recorded."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    dates = [0.5 * k for k in range(1, 5)]
    bm = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 4, 0.5), 3, 16_384, 4711)
    launches = lambda: gpu.engine_stats()["kernel_launches"]

    def run(flag):
        before = launches()
        out = mc.bermudan_max_call_mc(bm, [100.0, 100.0, 100.0], 0.05, 0.10, 0.20, dates, 100.0, basis_order=3, one_pass_basis=flag)
        return out, (launches() - before) / (len(dates) - 1)

    (value_off, error_off), per_date_off = run(False)
    (value_on, error_on), per_date_on = run(True)
    print(f"max-call, 3 assets, degree 3, 16384 paths: {value_on:.6f} ± {error_on:.6f}; launches per date {per_date_on:.1f} (one pass) / {per_date_off:.1f} (materialised)")
    assert value_on == value_off and error_on == error_off
    assert per_date_on < per_date_off


_DEVICES = r'''
import ctypes as C, importlib, json, sys
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
reg = importlib.import_module("finmath-lib-cuda-extensions_amd.regression")
mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
rng = np.random.default_rng(41)
n = 100_003
data = [np.exp(0.2 * rng.standard_normal(n)).astype(np.float32) for _ in range(3)]
extra = rng.standard_normal(n).astype(np.float32)
y = rng.standard_normal(n).astype(np.float32)
table = mc.monomial_exponents(3, 3)
beta = rng.standard_normal(len(table) + 1)

def ask(lo, hi):
    v = lambda a: fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(a[lo:hi]))
    states, ex, dep = [v(a) for a in data], [v(extra)], [v(y)]
    S, T = reg.polynomial_cross_moments(states, table, ex, dep)
    r = reg.polynomial_evaluate(states, table, beta, ex)
    return np.concatenate([S[np.triu_indices(S.shape[0])], T.ravel()]), r.to_float32()

groups = (n + 3) // 4                                  # the shards' ranges (shard_range: whole groups of four paths)
cut = min(((groups + 1) // 2) * 4, n)
fm.init(0)
first, second, (whole, values) = ask(0, cut)[0], ask(cut, n)[0], ask(0, n)
fm.shutdown()
fm.init_devices([0, 0])
sums, sharded = ask(0, n)
fm.shutdown()
print("RESULT " + json.dumps({"sums": bool(np.array_equal(sums.view(np.uint64), (first + second).view(np.uint64))), "n": float(sums[0]),
                              "close": float(np.abs(sums - whole).max() / np.abs(whole).max()),
                              "values": bool(np.array_equal(sharded.view(np.uint32), values.view(np.uint32))), "size": int(sharded.size)}))
'''


def test_device_list(tmp_path):
    """A device list [0, 0]: the sums are the two shards' single-device sums added in shard order, bit for bit; the evaluation is the
    single-device vector.  In a process of its own."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "devices.py"
    script.write_text(_DEVICES % {"root": root})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert out["sums"] and out["n"] == 100_003 and out["close"] < 1e-12
    assert out["values"] and out["size"] == 100_003
