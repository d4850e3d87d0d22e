"""Named functions and option formulas on the device (include/fmhip.h: fmhip_function_apply, fmhip_option_formula; csrc/analytic_kernel.hip;
DESIGN.md §4.21) on a real MI355X.  Every check of a kernel is an EQUALITY of bits with the host definition (fmhip_function_apply_host,
fmhip_option_formula_host): sizes around the kernels' group, tile and the wrap of their grid-stride loop (read from csrc/analytic_kernel.h),
each kind alone, the pair [Φ, φ], all three with a repeat, the edge inputs of tests/test_analytic_cpu.py at the first, a middle and the last
16-byte group; both models, every mask, the seven combinations of vector and scalar operands, degenerate elements among live ones, T = 0;
a pending x, operands unchanged afterwards, one launch and exactly the outputs in the pool, given-up values, the FMHIP_DEVICE_ANALYTIC=0
path and a device list of two shards in child processes, RandomVariableHip.apply, the AAD pair from one launch; the conditional Heston
driver against the closed form and against heston_call_mc, and the normal scores.  No test asks the device for anything out of range: bad
arguments are refused on the host before a launch."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_analytic_cpu import CDF, DENSITY, QUANTILE, apply_host, bits, edge_inputs, formula_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI32 = C.POINTER(C.c_int32)


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "analytic_kernel.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_ANALYTIC_\w+) = ([^;,]+)[;,]", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


K_ = header_constants()
BLOCK, TILE, MAX_BLOCKS = K_["FM_ANALYTIC_BLOCK"], K_["FM_ANALYTIC_TILE"], K_["FM_ANALYTIC_MAX_BLOCKS"]
assert TILE == BLOCK * 4                                                     # a lane takes one 16-byte group per iteration
WRAP = MAX_BLOCKS * TILE + 1                                                 # the smallest n whose grid-stride loop runs a second time in some lane
assert -(-WRAP // TILE) > MAX_BLOCKS and -(-(WRAP - 1) // TILE) == MAX_BLOCKS and WRAP + 3 < 4_000_000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, WRAP + 3, 100_003]
assert (TILE - 1) % 4 != 0 and (TILE + 1) % 4 != 0 and (WRAP + 3) % 4 == 0 and 100_003 % 4 != 0      # tails of 3, 1, 0 and 3 elements
KIND_SETS = [[CDF], [DENSITY], [QUANTILE], [CDF, DENSITY], [QUANTILE, DENSITY, CDF, QUANTILE]]


def sample(n, seed):
    """x over ±15 in the even positions, u over (0, 1) in the odd ones: every kind meets its domain and what lies outside."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-15.0, 15.0, n).astype(np.float32)
    x[1::2] = rng.uniform(0.0, 1.0, x[1::2].size).astype(np.float32)
    return x


def device_functions(gpu, v, kinds):
    kinds = np.array(kinds, dtype=np.int32)
    out = (C.c_int64 * kinds.size)()
    gpu._native.check(gpu.lib().fmhip_function_apply(v.handle, kinds.ctypes.data_as(PI32), kinds.size, out))
    return [gpu.DeviceVector(int(h), v.n).to_float32() for h in out]


def check_functions(gpu, x, kinds):
    v = gpu.DeviceVector.from_host(x)
    got, want = device_functions(gpu, v, kinds), apply_host(gpu, x, kinds)
    for f, (g, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero(bits(g) != bits(w))
        assert differ.size == 0, (x.size, kinds, f, differ[:5], x[differ[:5]], g[differ[:5]], w[differ[:5]])
    assert (bits(v.to_float32()) == bits(x)).all()                          # the pass only reads x


def device_formula(gpu, model, operands, T, K, mask):
    """fmhip_option_formula through ctypes: operands are DeviceVectors or floats; the columns in bit order."""
    handles = [o.handle if isinstance(o, gpu.DeviceVector) else 0 for o in operands]
    scalars = [0.0 if isinstance(o, gpu.DeviceVector) else float(o) for o in operands]
    n = next(o.n for o in operands if isinstance(o, gpu.DeviceVector))
    out = (C.c_int64 * bin(mask).count("1"))()
    gpu._native.check(gpu.lib().fmhip_option_formula(model, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], float(T), float(K), mask, out))
    return [gpu.DeviceVector(int(h), n).to_float32() for h in out]


def formula_operands(n, model, seed):
    """Forwards around the strike 100, volatilities (absolute ones for Bachelier), payoff units; degenerate and NaN elements among the live
    ones: σ = 0 and σ < 0, F = 0 and F < 0, ±inf, a NaN in each operand."""
    rng = np.random.default_rng(seed)
    F = rng.uniform(40.0, 180.0, n).astype(np.float32)
    sigma = (rng.uniform(0.01, 0.8, n) * (100.0 if model == 1 else 1.0)).astype(np.float32)
    unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    special = [(0, 0.0), (0, -3.0), (0, np.inf), (0, np.nan), (1, 0.0), (1, -0.2), (1, np.nan), (1, np.inf), (2, np.nan), (2, 0.0), (2, -1.0), (0, 1e-30), (1, 1e-6)]
    for j, (which, value) in enumerate(special):
        for at in ((7 * j) % n, (n // 2 + 5 * j) % n, (n - 1 - 3 * j) % n):
            (F, sigma, unit)[which][at] = value
    return F, sigma, unit


SCALARS = {0: (104.5, 0.3, 0.9), 1: (104.5, 30.0, 0.9)}


def check_formula(gpu, model, arrays, use_vector, T, K, mask):
    vectors = [gpu.DeviceVector.from_host(a) if use else None for a, use in zip(arrays, use_vector)]
    device_ops = [v if use else s for v, use, s in zip(vectors, use_vector, SCALARS[model])]
    host_ops = [a if use else s for a, use, s in zip(arrays, use_vector, SCALARS[model])]
    got, want = device_formula(gpu, model, device_ops, T, K, mask), formula_host(gpu, model, *host_ops, T, K, mask)
    assert len(got) == len(want) == bin(mask).count("1")
    for f, (g, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero(bits(g) != bits(w))
        assert differ.size == 0, (model, use_vector, T, mask, f, differ[:5], [a[differ[:5]] for a in arrays], g[differ[:5]], w[differ[:5]])
    for v, a in zip(vectors, arrays):
        if v is not None: assert (bits(v.to_float32()) == bits(a)).all()      # the pass only reads its operands


# ---------------------------------------------------------------- the unary kernel
@pytest.mark.parametrize("n", SIZES)
def test_every_size_equals_the_definition(gpu, n):
    x = sample(n, n)
    for kinds in KIND_SETS: check_functions(gpu, x, kinds)


def test_edge_inputs_in_the_first_a_middle_and_the_last_group(gpu):
    """±0, ±inf, NaN, denormals, the ends of the quantile's domain and beyond — starting at element 0, at a group in the middle and ending
    with the last element, of a vector whose last group is incomplete."""
    edges = edge_inputs()
    n = 100_003
    assert n % 4 == 3 and 3 * edges.size < n
    x = sample(n, 2)
    middle = (n // 2) // 4 * 4
    x[:edges.size] = edges; x[middle:middle + edges.size] = edges; x[n - edges.size:] = edges[::-1]
    assert np.isnan(x[n - edges.size:]).any() and np.isinf(x[:4 * ((edges.size + 3) // 4)]).any()
    for kinds in KIND_SETS: check_functions(gpu, x, kinds)


def test_arguments_on_and_beside_every_branch_of_the_definition(gpu):
    """The break points of Φ's pieces and the quantile's regions with their fp32 neighbours, and a dense sweep of the bit patterns."""
    from test_analytic_cpu import f32_between, mills_breaks, neighbours
    breaks = mills_breaks()
    x = np.concatenate([neighbours(breaks, 4), -neighbours(breaks, 4), neighbours([0.075, 0.925, 0.5, 1.3887944e-11], 4), f32_between(-40.0, 40.0, 50_000), f32_between(0.0, 1.0, 20_001)])
    for kinds in ([CDF, DENSITY, QUANTILE],): check_functions(gpu, x.astype(np.float32), kinds)


# ---------------------------------------------------------------- the formula kernel
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_of_the_formulas_equals_the_definition(gpu, model, n):
    arrays = formula_operands(n, model, n + model)
    check_formula(gpu, model, arrays, (True, True, True), 1.5, 100.0, 7)
    check_formula(gpu, model, arrays, (True, False, n % 2 == 0), 0.25, 100.0, 1 + n % 7)


@pytest.mark.parametrize("model", [0, 1])
def test_every_mask_and_every_combination_of_vector_and_scalar_operands(gpu, model):
    arrays = formula_operands(3 * TILE + 7, model, 17)
    for use_vector in itertools.product([True, False], repeat=3):
        if not any(use_vector): continue
        for mask in range(1, 8): check_formula(gpu, model, arrays, use_vector, 2.0, 100.0, mask)
    for mask in range(1, 8): check_formula(gpu, model, arrays, (True, True, True), 0.0, 100.0, mask)      # T = 0: every element is the limit
    check_formula(gpu, model, arrays, (True, True, True), 1.0, -5.0 if model == 1 else 0.0, 7)             # a strike that is degenerate under Black–Scholes


def test_refused_on_the_host_before_anything_runs(gpu):
    v = gpu.DeviceVector.from_host(np.ones(8, dtype=np.float32)); w = gpu.DeviceVector.from_host(np.ones(9, dtype=np.float32))
    before = gpu.pool_stats()
    out = (C.c_int64 * 4)()
    lib, E = gpu.lib(), gpu._native
    kinds = np.array([0, 1, 2, 3], dtype=np.int32)
    assert lib.fmhip_function_apply(v.handle, kinds.ctypes.data_as(PI32), 4, out) == E.ERR_INVALID_ARGUMENT           # kind 3
    assert lib.fmhip_function_apply(v.handle, kinds.ctypes.data_as(PI32), 0, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_function_apply(0, kinds.ctypes.data_as(PI32), 1, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_option_formula(0, 0, 100.0, 0, 0.2, 0, 1.0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT         # no vector
    assert lib.fmhip_option_formula(0, v.handle, 0.0, 0, 0.2, 0, 1.0, -1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_option_formula(0, v.handle, 0.0, 0, 0.2, 0, 1.0, 1.0, 100.0, 8, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_option_formula(2, v.handle, 0.0, 0, 0.2, 0, 1.0, 1.0, 100.0, 1, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_option_formula(0, v.handle, 0.0, w.handle, 0.0, 0, 1.0, 1.0, 100.0, 1, out) == E.ERR_SIZE_MISMATCH
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors and list(out) == [0] * 4


def test_a_pending_x_out_of_a_fused_chain(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = sample(TILE + 77, 1)
        stored = gpu.DeviceVector.from_host(base)
        pending = stored.v1s1("MULT_S", 0.5).v1s1("ADD_S", 0.25)           # nothing has run yet
        got = device_functions(gpu, pending, [CDF, DENSITY])
        x = pending.to_float32()
        assert (bits(x) == bits((base * np.float32(0.5) + np.float32(0.25)).astype(np.float32))).all()
        want = apply_host(gpu, x, [CDF, DENSITY])
        assert all((bits(g) == bits(w)).all() for g, w in zip(got, want))
        # two pending operands of a formula: one flush, then one launch
        F = stored.v1s1("MULT_S", 2.0).v1s1("ADD_S", 90.0); sigma = stored.v1s0("ABS").v1s1("MULT_S", 0.03)
        got = device_formula(gpu, 0, [F, sigma, 0.9], 1.5, 100.0, 7)
        want = formula_host(gpu, 0, F.to_float32(), sigma.to_float32(), 0.9, 1.5, 100.0, 7)
        assert all((bits(g) == bits(w)).all() for g, w in zip(got, want))
    finally:
        gpu.set_fusion(prev)


def test_one_launch_and_nothing_left_behind(gpu):
    v = gpu.DeviceVector.from_host(sample(5 * TILE + 3, 4))
    arrays = formula_operands(5 * TILE + 3, 0, 5)
    ops = [gpu.DeviceVector.from_host(a) for a in arrays]
    for kinds in KIND_SETS:
        kinds = np.array(kinds, dtype=np.int32)
        before = gpu.pool_stats()
        out = (C.c_int64 * kinds.size)()
        gpu._native.check(gpu.lib().fmhip_function_apply(v.handle, kinds.ctypes.data_as(PI32), kinds.size, out))
        kept = [gpu.DeviceVector(int(h), v.n) for h in out]
        after = gpu.pool_stats()
        assert after.n_kernel_launches == before.n_kernel_launches + 1 and after.n_live_vectors == before.n_live_vectors + kinds.size
        del kept
    for mask in range(1, 8):
        before = gpu.pool_stats()
        out = (C.c_int64 * 3)()
        gpu._native.check(gpu.lib().fmhip_option_formula(1, ops[0].handle, 0.0, ops[1].handle, 0.0, ops[2].handle, 0.0, 1.0, 100.0, mask, out))
        kept = [gpu.DeviceVector(int(h), v.n) for h in out if h]
        after = gpu.pool_stats()
        assert len(kept) == bin(mask).count("1")
        assert after.n_kernel_launches == before.n_kernel_launches + 1 and after.n_live_vectors == before.n_live_vectors + len(kept)
        del kept


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32) * np.float32(0.001))
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
                gpu.function_apply(y, [gpu.NORMAL_CDF])
                gpu.option_formula("bachelier", gpu.RandomVariableHip(0.0, base), gpu.RandomVariableHip(0.0, y), 1.0, 2.0)
            else:
                with pytest.raises(gpu.FmhipError) as info:
                    gpu.function_apply(y, [gpu.NORMAL_CDF])
                assert info.value.code == read_error and "given up" in str(info.value)
                with pytest.raises(gpu.FmhipError) as info:
                    gpu.option_formula("bachelier", gpu.RandomVariableHip(0.0, base), gpu.RandomVariableHip(0.0, y), 1.0, 2.0)
                assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


# ---------------------------------------------------------------- the knob and a device list, in child processes
_CHILD = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode, out_path = sys.argv[1], sys.argv[2]
data = dict(np.load(sys.argv[3]))
if mode == "devices_two": fm.init_devices([0, 0])
else: fm.init(0)
if mode == "knob_off": assert os.environ["FMHIP_DEVICE_ANALYTIC"] == "0"
fs = [fm.NORMAL_QUANTILE, fm.NORMAL_DENSITY, fm.NORMAL_CDF, fm.NORMAL_QUANTILE]
v = fm.DeviceVector.from_host(data["x"])
F, S, U = (fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(data[k])) for k in ("F", "S", "U"))
before = fm.pool_stats().n_kernel_launches
out = fm.function_apply(v, fs)
launches = fm.pool_stats().n_kernel_launches - before
pending = fm.function_apply(v.v1s1("MULT_S", 0.5), fs[1:3])
res = {"out%%d" %% f: o.to_float32() for f, o in enumerate(out)}
res.update({"pending%%d" %% f: o.to_float32() for f, o in enumerate(pending)})
before = fm.pool_stats().n_kernel_launches
bs = fm.option_formula("black_scholes", F, S, 1.5, 100.0, U, ("value", "delta", "vega"))
launches += fm.pool_stats().n_kernel_launches - before
ba = fm.option_formula("bachelier", F, 30.0, 0.25, 100.0, U, ("vega", "value"))
res.update({"bs%%d" %% f: o.realizations.to_float32() for f, o in enumerate(bs)})
res.update({"ba%%d" %% f: o.realizations.to_float32() for f, o in enumerate(ba)})
res["x"] = v.to_float32()
np.savez(out_path, **res)
print("LAUNCHES", launches)
fm.shutdown()
'''


@pytest.fixture(scope="module")
def child_case(gpu, tmp_path_factory):
    x = np.concatenate([edge_inputs(), sample(100_003, 8)])
    F, S, U = formula_operands(x.size, 0, 9)
    fs = [gpu.NORMAL_QUANTILE, gpu.NORMAL_DENSITY, gpu.NORMAL_CDF, gpu.NORMAL_QUANTILE]
    want = {f"out{f}": o for f, o in enumerate(gpu.function_apply_host(x, fs))}
    want.update({f"pending{f}": o for f, o in enumerate(gpu.function_apply_host((x * np.float32(0.5)).astype(np.float32), fs[1:3]))})
    want.update({f"bs{f}": o for f, o in enumerate(gpu.option_formula_host("black_scholes", F, S, 1.5, 100.0, U, ("value", "delta", "vega")))})
    want.update({f"ba{f}": o for f, o in enumerate(gpu.option_formula_host("bachelier", F, 30.0, 0.25, 100.0, U, ("vega", "value")))})
    want["x"] = x
    folder = tmp_path_factory.mktemp("analytic_children")
    np.savez(folder / "in.npz", x=x, F=F, S=S, U=U)
    (folder / "child.py").write_text(_CHILD % {"root": ROOT})
    return folder, want


@pytest.mark.parametrize("mode", ["device", "knob_off", "devices_two"])
def test_the_knob_and_a_device_list_give_the_same_bits(child_case, mode):
    """A fresh process on the device, one with FMHIP_DEVICE_ANALYTIC=0 (download, the definition on one core, upload: no launch of the
    kernels) and one behind fm.init_devices([0, 0]) (every shard its block): the bits of the definition, all three."""
    folder, want = child_case
    out_path = folder / (mode + ".npz")
    r = subprocess.run([sys.executable, str(folder / "child.py"), mode, str(out_path), str(folder / "in.npz")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FMHIP_DEVICE_ANALYTIC="0" if mode == "knob_off" else "1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    launches = int([line for line in r.stdout.splitlines() if line.startswith("LAUNCHES ")][-1].split()[1])
    res = dict(np.load(out_path))
    for name, w in want.items(): assert (bits(res[name]) == bits(w)).all(), (mode, name)
    if mode == "device": assert launches == 2                                # one per call
    if mode == "knob_off": assert launches == 0


# ---------------------------------------------------------------- the mirrors
def test_random_variable_apply_keeps_the_time_and_maps_a_constant(gpu):
    x = sample(4 * TILE + 5, 3)
    rv = gpu.RandomVariableHip(1.25, x)
    for f, kind in ((gpu.NORMAL_CDF, CDF), (gpu.NORMAL_DENSITY, DENSITY), (gpu.NORMAL_QUANTILE, QUANTILE)):
        y = rv.apply(f)
        assert isinstance(y, gpu.RandomVariableHip) and y.getFiltrationTime() == 1.25 and not y.isDeterministic() and y.size() == x.size
        assert (bits(y.realizations.to_float32()) == bits(apply_host(gpu, x, [kind])[0])).all()
    c = gpu.RandomVariableHip(0.5, 0.3).apply(gpu.NORMAL_CDF)
    assert c.isDeterministic() and c.getFiltrationTime() == 0.5 and c.value == gpu.NORMAL_CDF(0.3)
    with pytest.raises(NotImplementedError): rv.apply(abs)
    F, S, U = formula_operands(x.size, 0, 4)
    value, vega = gpu.option_formula("black_scholes", gpu.RandomVariableHip(0.5, F), gpu.RandomVariableHip(2.0, S), 1.5, 100.0, gpu.RandomVariableHip(1.0, U), ("value", "vega"))
    assert value.getFiltrationTime() == vega.getFiltrationTime() == 2.0     # the operands' maximum
    want = gpu.option_formula_host("black_scholes", F, S, 1.5, 100.0, U, ("value", "vega"))
    assert (bits(value.realizations.to_float32()) == bits(want[0])).all() and (bits(vega.realizations.to_float32()) == bits(want[1])).all()
    mixed = gpu.bachelier_option_value(gpu.RandomVariableHip(0.5, F), 30.0, 1.5, 100.0, gpu.RandomVariableHip(3.0, 0.9))      # a deterministic operand is a scalar
    assert mixed.getFiltrationTime() == 3.0 and (bits(mixed.realizations.to_float32()) == bits(gpu.option_formula_host("bachelier", F, 30.0, 1.5, 100.0, 0.9)[0])).all()


def test_aad_value_and_derivative_come_from_one_launch(gpu):
    x = sample(2 * TILE + 9, 5)
    factory = gpu.RandomVariableDifferentiableAADFactory(gpu.RandomVariableHipFactory())
    X = factory.createRandomVariable(0.0, x)
    X.getValues().realizations.to_float32()                                  # x is stored: nothing of it is pending
    before = gpu.pool_stats().n_kernel_launches
    Y = X.apply(gpu.NORMAL_CDF)
    assert gpu.pool_stats().n_kernel_launches == before + 1                  # value AND derivative: one read of x
    value, slope = apply_host(gpu, x, [CDF, DENSITY])
    assert (bits(Y.getValues().realizations.to_float32()) == bits(value)).all()
    g = Y.average().getGradient()[X.getID()]
    assert (bits(np.broadcast_to(g.getRealizations(), x.shape)) == bits(slope)).all()
    # the formula with AAD operands: ONE launch gives the unit value and both partials
    F, S, U = formula_operands(x.size, 0, 6)
    F, S, U = np.abs(np.nan_to_num(F, nan=100.0, posinf=120.0)) + 1, np.abs(np.nan_to_num(S, nan=0.2, posinf=0.3)) + np.float32(0.01), np.nan_to_num(U, nan=1.0)
    f, s, u = (factory.createRandomVariable(0.0, a.astype(np.float32)) for a in (F, S, U))
    for v in (f, s, u): v.getValues().realizations.to_float32()
    before = gpu.pool_stats().n_kernel_launches
    value, = gpu.option_formula("black_scholes", f, s, 1.5, 100.0, 1.0)
    assert gpu.pool_stats().n_kernel_launches == before + 1
    v1, d1, g1 = gpu.option_formula_host("black_scholes", F, S, 1.5, 100.0, 1.0, ("value", "delta", "vega"))
    assert (bits(value.getValues().realizations.to_float32()) == bits(v1)).all()
    gradient = gpu.option_formula("black_scholes", f, s, 1.5, 100.0, u)[0].average().getGradient()
    assert np.allclose(gradient[f.getID()].getRealizations(), d1 * U, rtol=3e-7, atol=1e-30) and np.allclose(gradient[s.getID()].getRealizations(), g1 * U, rtol=3e-7, atol=1e-30)
    assert (bits(gradient[u.getID()].getRealizations()) == bits(v1)).all()


# ---------------------------------------------------------------- the drivers: 2^16 paths, 50 steps
PATHS, STEPS = 1 << 16, 50


def brownian(gpu, factors, seed=31415):
    return gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, STEPS, 1.0 / STEPS), factors, PATHS, seed)


def test_conditional_heston_without_vol_of_vol_is_the_closed_form_on_every_path(gpu):
    """ξ = 0 and v0 = θ: the variance stays θ, I = Σ θ Δt, J is multiplied by ρ and ρ²I/2 is taken off: with ρ = 0 every path is the
    Black–Scholes value at σ² = I/T.  I is a sum of 50 fp32 terms: within 50·2^-24 relative of the closed form."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    average, vector = mc.heston_call_conditional_mc(brownian(gpu, 1), 100.0, 0.05, 0.04, 1.5, 0.04, 0.0, 0.0, 1.0, 100.0)
    exact = mc.black_scholes_call_analytic(100.0, 0.05, 0.2, 1.0, 100.0)
    values = vector.realizations.to_float32() if not vector.isDeterministic() else np.array([vector.value])
    print(f"conditional Heston, xi = 0: {average!r}, Black-Scholes {exact!r}, spread over the paths {float(values.max() - values.min())!r}")
    assert values.max() == values.min()
    assert abs(average - exact) <= 50 * 2.0 ** -24 * exact
    # the same with ρ = −0.7: the forwards differ from path to path, the law does not: the same closed form within 3 standard errors
    average, vector = mc.heston_call_conditional_mc(brownian(gpu, 1), 100.0, 0.05, 0.04, 1.5, 0.04, 0.0, -0.7, 1.0, 100.0)
    err = vector.getStandardError()
    print(f"conditional Heston, xi = 0, rho = -0.7: {average:.5f} +- {err:.5f}")
    assert 0.0 < err < 0.05 and abs(average - exact) <= 3 * err


def test_conditional_heston_agrees_with_the_plain_driver_and_has_less_variance(gpu):
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    parameters = (100.0, 0.05, 0.04, 1.5, 0.04, 0.5, -0.7, 1.0, 100.0)
    conditional, c_vector = mc.heston_call_conditional_mc(brownian(gpu, 1, seed=271828), *parameters)
    plain, p_vector = mc.heston_call_mc(brownian(gpu, 2), *parameters)
    c_err, p_err = c_vector.getStandardError(), p_vector.getStandardError()
    print(f"Heston call: conditional {conditional:.5f} +- {c_err:.5f}, plain {plain:.5f} +- {p_err:.5f}, standard-error ratio {p_err / c_err:.2f}, variance ratio {(p_err / c_err) ** 2:.1f}")
    assert 0.0 < c_err < p_err
    assert abs(conditional - plain) <= 3 * math.hypot(c_err, p_err)


def test_normal_scores_have_mean_zero_and_the_order_of_the_input(gpu):
    x = np.random.default_rng(77).standard_t(3, PATHS).astype(np.float32)
    v = gpu.DeviceVector.from_host(x)
    scores = gpu.normal_scores(v).to_float32()
    assert np.isfinite(scores).all() and abs(float(scores.astype(np.float64).mean())) <= 1e-6
    assert (np.argsort(scores, kind="stable") == np.argsort(x, kind="stable")).all()
    rv = gpu.RandomVariableHip(0.75, gpu.rank_scores(v)).apply(gpu.NORMAL_QUANTILE)                  # normal_scores is this composition
    assert (bits(rv.realizations.to_float32()) == bits(scores)).all()
