"""Tabulated functions on the device (include/fmhip.h: fmhip_table_apply; csrc/table_kernel.hip) on a real MI355X.  Every check
of the kernel is an EQUALITY with fmhip_table_apply_host, the definition: sizes around the kernel's group, tile and the wrap of its
grid-stride loop (read from csrc/table_kernel.h), 1 … 1024 knots in three families, 1 … 4 tables per call up to the knots x tables limit,
the edge inputs of tests/test_table_cpu.py at the first, a middle and the last 16-byte group, a pending x, x unchanged afterwards, the
FMHIP_DEVICE_TABLE=0 path and a device list of two shards in child processes, RandomVariableHip.apply, the AAD pair from one launch, and a
local-volatility Monte-Carlo against Black–Scholes.  No test asks the device for anything out of range: bad arguments are refused on the
host before a launch."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_table_cpu import KNOT_COUNTS, PD, apply_host, bits, build, edge_inputs, values_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "table_kernel.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_TABLE_\w+) = ([^;,]+)[;,]", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


K_ = header_constants()
BLOCK, TILE, MAX_BLOCKS = K_["FM_TABLE_BLOCK"], K_["FM_TABLE_TILE"], K_["FM_TABLE_MAX_BLOCKS"]
assert TILE == BLOCK * 4                                                     # a lane takes one 16-byte group per iteration
WRAP = MAX_BLOCKS * TILE + 1                                                 # the smallest n whose grid-stride loop runs a second time in some lane
assert -(-WRAP // TILE) > MAX_BLOCKS and -(-(WRAP - 1) // TILE) == MAX_BLOCKS and WRAP + 3 < 4_000_000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, WRAP + 3, 100_003]
assert (TILE - 1) % 4 != 0 and (TILE + 1) % 4 != 0 and (WRAP + 3) % 4 == 0 and 100_003 % 4 != 0      # tails of 3, 1, 0 and 3 elements


def knots_of(m, kind):
    i = np.arange(m, dtype=np.float64)
    if kind == "uniform": return 0.1 * i - 1.7
    if kind == "geometric": return 1e-6 * 1e12 ** (i / max(m - 1, 1))
    if kind == "clusters": return np.where(i < m // 2, -100.0 + 1e-3 * i, 100.0 + 1e-3 * i)
    raise ValueError(kind)


def sample(n, K, seed):
    """Across the knots' range and a tenth beyond on both sides, every seventh element ON a knot (narrowed to fp32)."""
    rng = np.random.default_rng(seed)
    span = max(K[-1] - K[0], 1.0)
    x = rng.uniform(K[0] - 0.1 * span, K[-1] + 0.1 * span, n).astype(np.float32)
    on = np.arange(3, n, 7)
    x[on] = K[rng.integers(0, K.size, on.size)].astype(np.float32)
    return x


def tables(fm, K, T, seed=0):
    return np.stack([build(fm, K, values_of(K, seed + f), (seed + f) % 4, ((seed + f) // 2) % 2, 1 if f == 3 else 0) for f in range(T)])


def device(gpu, v, K, coefs):
    """fmhip_table_apply through ctypes: (T, n) float32."""
    K = np.ascontiguousarray(K, dtype=np.float64); coefs = np.ascontiguousarray(coefs, dtype=np.float64)
    T = coefs.shape[0]
    out = (C.c_int64 * T)()
    gpu._native.check(gpu.lib().fmhip_table_apply(v.handle, K.ctypes.data_as(PD), K.size, coefs.ctypes.data_as(PD), T, out))
    return np.stack([gpu.DeviceVector(int(h), v.n).to_float32() for h in out])


def check(gpu, x, K, coefs):
    v = gpu.DeviceVector.from_host(x)
    got, want = device(gpu, v, K, coefs), apply_host(gpu, x, K, coefs)
    for f in range(coefs.shape[0]):
        differ = np.flatnonzero(bits(got[f]) != bits(want[f]))
        assert differ.size == 0, (x.size, K.size, f, differ[:5], x[differ[:5]], got[f][differ[:5]], want[f][differ[:5]])
    assert (bits(v.to_float32()) == bits(x)).all()                          # the pass only reads x


@pytest.mark.parametrize("n", SIZES)
def test_every_size_equals_the_definition(gpu, n):
    for m, kind, T in ((65, "geometric", 2), (1024, "uniform", 1), (5, "clusters", 4)):
        K = knots_of(m, kind)
        check(gpu, sample(n, K, n + m), K, tables(gpu, K, T, seed=m))


@pytest.mark.parametrize("kind", ["uniform", "geometric", "clusters"])
@pytest.mark.parametrize("m", KNOT_COUNTS)
def test_every_number_of_knots_and_tables_equals_the_definition(gpu, m, kind):
    K = knots_of(m, kind)
    x = np.concatenate([edge_inputs(K), sample(TILE + 1, K, m)])
    for T in (1, 2, 4):
        if m * T > 1024: continue
        check(gpu, x, K, tables(gpu, K, T, seed=T))


@pytest.mark.parametrize("m, T", [(1024, 1), (512, 2), (256, 4)])
def test_the_knots_times_tables_limit(gpu, m, T):
    assert m * T == 1024
    for kind in ("uniform", "geometric", "clusters"):
        K = knots_of(m, kind)
        check(gpu, sample(3 * TILE + 1, K, m + T), K, tables(gpu, K, T, seed=1))
    K = knots_of(m + 1, "uniform")                                         # one knot more: refused on the host, nothing launched
    v = gpu.DeviceVector.from_host(np.zeros(8, dtype=np.float32))
    before = gpu.pool_stats().n_kernel_launches
    out = (C.c_int64 * 4)()
    coefs = np.zeros((T, m + 2, 4))
    assert gpu.lib().fmhip_table_apply(v.handle, K.ctypes.data_as(PD), m + 1, coefs.ctypes.data_as(PD), T, out) == gpu._native.ERR_INVALID_ARGUMENT
    assert gpu.pool_stats().n_kernel_launches == before and list(out) == [0] * 4


@pytest.mark.parametrize("m, kind", [(5, "uniform"), (64, "geometric"), (1023, "clusters")])
def test_edge_inputs_in_the_first_a_middle_and_the_last_group(gpu, m, kind):
    """Every knot and its fp32 neighbours, beyond both ends, ±0, ±inf, NaN, denormals — starting at element 0, at a group in the middle and
    ending with the last element, of a vector whose last group is incomplete."""
    K = knots_of(m, kind)
    edges = edge_inputs(K)
    n = 100_003
    assert n % 4 == 3 and 3 * edges.size < n
    x = sample(n, K, m)
    middle = (n // 2) // 4 * 4
    x[:edges.size] = edges; x[middle:middle + edges.size] = edges; x[n - edges.size:] = edges[::-1]
    assert np.isnan(x[n - edges.size:]).any() and np.isinf(x[:4 * ((edges.size + 3) // 4)]).any()
    check(gpu, x, K, tables(gpu, K, min(4, 1024 // m), seed=2))


def test_a_pending_x_out_of_a_fused_chain(gpu):
    prev = gpu.set_fusion(True)
    try:
        K = knots_of(33, "uniform")
        coefs = tables(gpu, K, 2)
        base = sample(TILE + 77, K, 1)
        stored = gpu.DeviceVector.from_host(base)
        pending = stored.v1s1("MULT_S", 0.5).v1s1("ADD_S", 0.25)           # nothing has run yet
        got = device(gpu, pending, K, coefs)
        x = pending.to_float32()
        assert (bits(x) == bits((base * np.float32(0.5) + np.float32(0.25)).astype(np.float32))).all()
        want = apply_host(gpu, x, K, coefs)
        assert (bits(got) == bits(want)).all()
        assert (bits(device(gpu, pending, K, coefs)) == bits(want)).all()   # and again, now that it is stored
    finally:
        gpu.set_fusion(prev)


def test_one_launch_and_nothing_left_behind(gpu):
    K = knots_of(64, "geometric")
    v = gpu.DeviceVector.from_host(sample(5 * TILE + 3, K, 4))
    for T in (1, 2, 3, 4):
        coefs = tables(gpu, K, T)
        gpu.table_apply(v, [gpu.TabulatedFunction(K, values_of(K, 0))])      # (scratch and stage are sized)
        before = gpu.pool_stats()
        out = (C.c_int64 * T)()
        gpu._native.check(gpu.lib().fmhip_table_apply(v.handle, K.ctypes.data_as(PD), K.size, coefs.ctypes.data_as(PD), T, out))
        kept = [gpu.DeviceVector(int(h), v.n) for h in out]
        after = gpu.pool_stats()
        assert after.n_kernel_launches == before.n_kernel_launches + 1 and after.n_live_vectors == before.n_live_vectors + T
        del kept


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        f = gpu.TabulatedFunction([0.0, 1000.0, 5000.0], [1.0, 2.0, 0.0])
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
            if read_error is None:
                gpu.table_apply(y, [f])
            else:
                with pytest.raises(gpu.FmhipError) as info:
                    gpu.table_apply(y, [f])
                assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


# ---------------------------------------------------------------- the knob and a device list, in child processes
_CHILD = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode, out_path = sys.argv[1], sys.argv[2]
data = dict(np.load(sys.argv[3]))
if mode == "devices_two": fm.init_devices([0, 0])
else: fm.init(0)
if mode == "knob_off": assert os.environ["FMHIP_DEVICE_TABLE"] == "0"
fs = [fm.TabulatedFunction(data["K"], data["V%%d" %% f], ["piecewise_constant", "linear", "cubic_spline", "monotone_cubic"][f], ["constant", "linear"][f %% 2]) for f in range(3)]
fs.append(fs[2].derivative())
v = fm.DeviceVector.from_host(data["x"])
before = fm.pool_stats().n_kernel_launches
out = fm.table_apply(v, fs)
launches = fm.pool_stats().n_kernel_launches - before
pending = fm.table_apply(v.v1s1("MULT_S", 0.5), fs[:2])
res = {"out%%d" %% f: o.to_float32() for f, o in enumerate(out)}
res.update({"pending%%d" %% f: o.to_float32() for f, o in enumerate(pending)})
res["x"] = v.to_float32()
np.savez(out_path, **res)
print("LAUNCHES", launches)
fm.shutdown()
'''


@pytest.fixture(scope="module")
def child_case(gpu, tmp_path_factory):
    K = knots_of(65, "geometric")
    x = np.concatenate([edge_inputs(K), sample(100_003, K, 8)])
    data = {"K": K, "x": x, **{f"V{f}": values_of(K, f) for f in range(3)}}
    fs = [gpu.TabulatedFunction(K, data[f"V{f}"], ["piecewise_constant", "linear", "cubic_spline", "monotone_cubic"][f], ["constant", "linear"][f % 2]) for f in range(3)]
    fs.append(fs[2].derivative())
    want = gpu.table_apply_host(x, fs)
    want_pending = gpu.table_apply_host((x * np.float32(0.5)).astype(np.float32), fs[:2])
    got = [o.to_float32() for o in gpu.table_apply(gpu.DeviceVector.from_host(x), fs)]
    for g, w in zip(got, want): assert (bits(g) == bits(w)).all()
    folder = tmp_path_factory.mktemp("table_children")
    np.savez(folder / "in.npz", **data)
    (folder / "child.py").write_text(_CHILD % {"root": ROOT})
    return folder, x, want, want_pending


def run_child(folder, mode, env):
    out_path = folder / (mode + ".npz")
    r = subprocess.run([sys.executable, str(folder / "child.py"), mode, str(out_path), str(folder / "in.npz")], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    launches = int([line for line in r.stdout.splitlines() if line.startswith("LAUNCHES ")][-1].split()[1])
    return launches, dict(np.load(out_path))


@pytest.mark.parametrize("mode", ["device", "knob_off", "devices_two"])
def test_the_knob_and_a_device_list_give_the_same_bits(child_case, mode):
    """A fresh process on the device, one with FMHIP_DEVICE_TABLE=0 (download, the definition on one core, upload: no launch of the kernel)
    and one behind fm.init_devices([0, 0]) (every shard its block): the bits of the definition, all three."""
    folder, x, want, want_pending = child_case
    launches, res = run_child(folder, mode, {"FMHIP_DEVICE_TABLE": "0" if mode == "knob_off" else "1"})
    for f, w in enumerate(want): assert (bits(res[f"out{f}"]) == bits(w)).all(), (mode, f)
    for f, w in enumerate(want_pending): assert (bits(res[f"pending{f}"]) == bits(w)).all(), (mode, f)
    assert (bits(res["x"]) == bits(x)).all()
    if mode == "device": assert launches == 1
    if mode == "knob_off": assert launches == 0


# ---------------------------------------------------------------- the mirrors
def test_random_variable_apply_keeps_the_time_and_maps_a_constant(gpu):
    K = knots_of(17, "uniform"); V = values_of(K, 6)
    f = gpu.TabulatedFunction(K, V, "cubic_spline", "linear")
    x = sample(4 * TILE + 5, K, 3)
    rv = gpu.RandomVariableHip(1.25, x)
    y = rv.apply(f)
    assert isinstance(y, gpu.RandomVariableHip) and y.getFiltrationTime() == 1.25 and not y.isDeterministic() and y.size() == x.size
    assert (bits(y.realizations.to_float32()) == bits(gpu.table_apply_host(x, [f])[0])).all()
    c = gpu.RandomVariableHip(0.5, 0.3).apply(f)
    assert c.isDeterministic() and c.getFiltrationTime() == 0.5 and c.value == f(0.3)
    with pytest.raises(NotImplementedError): rv.apply(abs)
    with pytest.raises(NotImplementedError): rv.apply(lambda v: v)


def test_aad_value_and_derivative_come_from_one_launch(gpu):
    K = knots_of(33, "uniform"); V = values_of(K, 7)
    f = gpu.TabulatedFunction(K, V, "monotone_cubic", "linear")
    x = sample(2 * TILE + 9, K, 5)
    factory = gpu.RandomVariableDifferentiableAADFactory(gpu.RandomVariableHipFactory())
    X = factory.createRandomVariable(0.0, x)
    X.getValues().realizations.to_float32()                                  # x is stored: nothing of it is pending
    gpu.table_apply(X.getValues().realizations, [f, f.derivative()])         # (scratch and stage are sized)
    before = gpu.pool_stats().n_kernel_launches
    Y = X.apply(f)
    assert gpu.pool_stats().n_kernel_launches == before + 1                  # value AND derivative: one read of x
    value, slope = gpu.table_apply_host(x, [f, f.derivative()])
    assert (bits(Y.getValues().realizations.to_float32()) == bits(value)).all()
    g = Y.average().getGradient()[X.getID()]
    assert (bits(np.broadcast_to(g.getRealizations(), x.shape)) == bits(slope)).all()
    with pytest.raises(NotImplementedError): X.apply(abs)


# ---------------------------------------------------------------- a local-volatility Euler scheme that never leaves the device
PATHS = 1 << 18
SPOTS = np.linspace(20.0, 300.0, 57)


def local_volatility(gpu, times, vols, seed=31415):
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    bm = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 8, 0.125), 1, PATHS, seed)
    return mc, mc.local_volatility_call_mc(bm, 100.0, 0.05, times, SPOTS, vols, 1.0, 100.0)


def test_a_flat_surface_is_black_scholes(gpu):
    mc, (value, err) = local_volatility(gpu, [0.0], np.full((1, SPOTS.size), 0.2))
    exact = mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)
    print(f"flat surface: {value:.5f} +- {err:.5f}, Black-Scholes {exact:.5f}")
    assert 0.0 < err < 0.05 and abs(value - exact) <= 3 * err


def test_a_surface_that_depends_on_time_only_is_black_scholes_at_the_rms_volatility(gpu):
    times = [0.0, 0.25, 0.5, 0.75]
    sig = np.array([0.15, 0.3, 0.1, 0.25])
    mc, (value, err) = local_volatility(gpu, times, np.repeat(sig[:, None], SPOTS.size, axis=1))
    rms = math.sqrt(float(np.mean(sig ** 2)))                               # four quarters of equal length, maturity 1
    exact = mc.black_scholes_call_analytic(100.0, 0.05, rms, 1.0, 100.0)
    print(f"time-dependent surface: {value:.5f} +- {err:.5f}, Black-Scholes at {rms:.5f}: {exact:.5f}")
    assert 0.0 < err < 0.05 and abs(value - exact) <= 3 * err


def test_a_skewed_surface_is_the_same_on_the_device_and_on_the_host_path(gpu, monkeypatch):
    times = [0.0, 0.5]
    vols = np.stack([0.2 + 0.15 * (100.0 - SPOTS) / 100.0, 0.25 + 0.1 * (100.0 - SPOTS) / 100.0]).clip(0.05, 0.6)
    monkeypatch.setenv("FMHIP_DEVICE_TABLE", "1")
    launches = gpu.pool_stats().n_kernel_launches
    _, on_device = local_volatility(gpu, times, vols)
    assert gpu.pool_stats().n_kernel_launches > launches
    monkeypatch.setenv("FMHIP_DEVICE_TABLE", "0")
    _, on_host = local_volatility(gpu, times, vols)
    assert np.array(on_device).view(np.uint64).tolist() == np.array(on_host).view(np.uint64).tolist(), (on_device, on_host)
    _, flat = local_volatility(gpu, [0.0], np.full((1, SPOTS.size), 0.2))
    assert on_device[0] != flat[0]                                            # the skew is in the value
