"""Implied volatility per path on the device (include/fmhip.h: fmhip_implied_volatility; csrc/implied_volatility_kernel.hip)
on a real MI355X.  Every check of the kernel is an EQUALITY of bits with the host definition (fmhip_implied_volatility_host): sizes around
the kernel's group, tile and the wrap of its grid-stride loop (read from csrc/implied_volatility_kernel.h), both models, every mask, the
seven combinations of vector and scalar operands, prices made by option_formula from random volatilities with the edge list of
tests/test_implied_volatility_cpu.py planted in the first, a middle and the last group, T = 0; pending operands computed in one flush and
one launch for the call, exactly the outputs in the pool, given-up values, the FMHIP_DEVICE_ANALYTIC=0 path and a device list of two shards
in child processes, the mirrors, the AAD triple from one launch, and the forward-smile driver: without vol of vol against the volatility
it was given and against its numpy restatement on the same draws, with vol of vol against its run with the knobs off.  No test
asks the device for anything out of range: bad arguments are refused on the host before a launch."""
import ctypes as C
import itertools
import json
import math
import os
import re
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_implied_volatility_cpu import DRIVER_CASE, bits, edge_rows, implied_host, restated_forward_smile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "black_scholes", 1: "bachelier"}


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "implied_volatility_kernel.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_IMPLIED_\w+) = ([^;,]+)[;,]", text):
        env[name] = int(eval(expr, {"__builtins__": {}}, env))
    return env


K_ = header_constants()
BLOCK, TILE, MAX_BLOCKS = K_["FM_IMPLIED_BLOCK"], K_["FM_IMPLIED_TILE"], K_["FM_IMPLIED_MAX_BLOCKS"]
assert TILE == BLOCK * 4                                                     # a lane takes one 16-byte group per iteration
WRAP = MAX_BLOCKS * TILE + 1                                                 # the smallest n whose grid-stride loop runs a second time in some lane
assert -(-WRAP // TILE) > MAX_BLOCKS and -(-(WRAP - 1) // TILE) == MAX_BLOCKS and WRAP + 3 < 4_000_000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, WRAP + 3, 100_003]
SCALARS = (9.25, 104.5, 0.9)


def operands(gpu, n, model, seed, T=1.5, K=100.0):
    """Prices made by option_formula from random volatilities at forwards around the strike and payoff units around 1, with the edge list
    planted in the first, a middle and the last group where the vector is long enough, and singly, strided, where it is not."""
    rng = np.random.default_rng(seed)
    F = rng.uniform(40.0, 180.0, n).astype(np.float32)
    sigma = (rng.uniform(0.05, 0.8, n) * (100.0 if model == 1 else 1.0)).astype(np.float32)
    unit = rng.uniform(0.5, 1.5, n).astype(np.float32)
    P = gpu.option_formula_host(NAMES[model], F, sigma, T, K, unit)[0]
    rows = edge_rows(model)
    if n >= 3 * len(rows):
        middle = (n // 2) // 4 * 4
        for start in (0, middle, n - len(rows)):
            for i, (price, forward, payoff_unit, _) in enumerate(rows): P[start + i], F[start + i], unit[start + i] = price, forward, payoff_unit
    else:
        for i, (price, forward, payoff_unit, _) in enumerate(rows[:n]):
            if (i + seed) % 3 == 0: P[i], F[i], unit[i] = price, forward, payoff_unit
    return P, F, unit


def device_implied(gpu, model, ops, T, K, mask):
    """fmhip_implied_volatility through ctypes: operands are DeviceVectors or floats; the columns in bit order."""
    handles = [o.handle if isinstance(o, gpu.DeviceVector) else 0 for o in ops]
    scalars = [0.0 if isinstance(o, gpu.DeviceVector) else float(o) for o in ops]
    n = next(o.n for o in ops if isinstance(o, gpu.DeviceVector))
    out = (C.c_int64 * bin(mask).count("1"))()
    gpu._native.check(gpu.lib().fmhip_implied_volatility(model, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], float(T), float(K), mask, out))
    return [gpu.DeviceVector(int(h), n).to_float32() for h in out]


def check(gpu, model, arrays, use_vector, T, K, mask):
    vectors = [gpu.DeviceVector.from_host(a) if use else None for a, use in zip(arrays, use_vector)]
    device_ops = [v if use else s for v, use, s in zip(vectors, use_vector, SCALARS)]
    host_ops = [a if use else s for a, use, s in zip(arrays, use_vector, SCALARS)]
    got, want = device_implied(gpu, model, device_ops, T, K, mask), implied_host(gpu, model, *host_ops, T, K, mask)
    assert len(got) == len(want) == bin(mask).count("1")
    for f, (g, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero(bits(g) != bits(w))
        assert differ.size == 0, (model, use_vector, T, mask, f, differ[:5], [a[differ[:5]] for a in arrays], g[differ[:5]], w[differ[:5]])
    for v, a in zip(vectors, arrays):
        if v is not None: assert (bits(v.to_float32()) == bits(a)).all()      # the pass only reads its operands


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_equals_the_definition(gpu, model, n):
    arrays = operands(gpu, n, model, n + model)
    check(gpu, model, arrays, (True, True, True), 1.5, 100.0, 7)
    check(gpu, model, arrays, (True, n % 2 == 0, False), 1.5, 100.0, 1 + n % 7)


@pytest.mark.parametrize("model", [0, 1])
def test_every_mask_and_every_combination_of_vector_and_scalar_operands(gpu, model):
    arrays = operands(gpu, 3 * TILE + 7, model, 17, T=2.0)
    for use_vector in itertools.product([True, False], repeat=3):
        if not any(use_vector): continue
        for mask in range(1, 8): check(gpu, model, arrays, use_vector, 2.0, 100.0, mask)
    for mask in (1, 7): check(gpu, model, arrays, (True, True, True), 0.0, 100.0, mask)      # T = 0: +0 without a time value, a NaN with one
    check(gpu, model, arrays, (True, True, True), 1.0, -5.0 if model == 1 else 0.0, 7)        # a strike that is no strike under Black–Scholes


def test_the_edge_list_is_where_it_was_planted(gpu):
    """The planted elements answer what the semantics state, on the device: the equality above compares with a host that could share a mistake."""
    for model in (0, 1):
        n = 100_003
        P, F, unit = operands(gpu, n, model, 3, T=1.0)
        sigma, d_price, d_forward = device_implied(gpu, model, [gpu.DeviceVector.from_host(a) for a in (P, F, unit)], 1.0, 100.0, 7)
        rows = edge_rows(model)
        for start in (0, (n // 2) // 4 * 4, n - len(rows)):
            for i, (_, _, _, what) in enumerate(rows):
                p = start + i
                if what == "live": assert sigma[p] > 0 and np.isfinite(sigma[p]) and d_price[p] > 0 and d_forward[p] < 0
                else: assert bits(sigma[p:p + 1])[0] == {"nan": 0x7fc00000, "zero": 0, "inf": 0x7f800000}[what] and bits(d_price[p:p + 1])[0] == 0x7fc00000 and bits(d_forward[p:p + 1])[0] == 0x7fc00000


def test_refused_on_the_host_before_anything_runs(gpu):
    v = gpu.DeviceVector.from_host(np.full(8, 8.0, dtype=np.float32)); w = gpu.DeviceVector.from_host(np.ones(9, dtype=np.float32))
    before = gpu.pool_stats()
    out = (C.c_int64 * 3)()
    lib, E = gpu.lib(), gpu._native
    assert lib.fmhip_implied_volatility(0, 0, 8.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT         # no vector
    assert lib.fmhip_implied_volatility(0, v.handle, 0.0, 0, 100.0, 0, 1.0, -1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_implied_volatility(0, v.handle, 0.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 8, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_implied_volatility(0, v.handle, 0.0, 0, 100.0, 0, 1.0, 1.0, float("nan"), 1, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_implied_volatility(2, v.handle, 0.0, 0, 100.0, 0, 1.0, 1.0, 100.0, 1, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_implied_volatility(0, v.handle, 0.0, w.handle, 0.0, 0, 1.0, 1.0, 100.0, 1, out) == E.ERR_SIZE_MISMATCH
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors and list(out) == [0] * 3


def test_pending_operands_are_computed_in_one_flush_and_the_call_is_one_launch(gpu):
    prev = gpu.set_fusion(True)
    try:
        rng = np.random.default_rng(1)
        base = rng.uniform(60.0, 140.0, TILE + 77).astype(np.float32)
        stored = gpu.DeviceVector.from_host(base)
        price = stored.v1s1("MULT_S", 0.05).v1s1("ADD_S", 4.0); forward = stored.v1s1("MULT_S", 0.1).v1s1("ADD_S", 90.0)      # nothing has run yet
        before = gpu.pool_stats().n_kernel_launches
        got = device_implied(gpu, 0, [price, forward, 0.9], 1.5, 100.0, 7)
        flushed = gpu.pool_stats().n_kernel_launches - before
        want = implied_host(gpu, 0, price.to_float32(), forward.to_float32(), 0.9, 1.5, 100.0, 7)
        assert all((bits(g) == bits(w)).all() for g, w in zip(got, want)) and np.isfinite(want[0]).sum() > TILE // 2
        # stored operands: exactly one launch, exactly the outputs in the pool
        ops = [gpu.DeviceVector.from_host(a) for a in operands(gpu, 5 * TILE + 3, 1, 5)]
        for mask in range(1, 8):
            before = gpu.pool_stats()
            out = (C.c_int64 * 3)()
            gpu._native.check(gpu.lib().fmhip_implied_volatility(1, ops[0].handle, 0.0, ops[1].handle, 0.0, ops[2].handle, 0.0, 1.5, 100.0, mask, out))
            kept = [gpu.DeviceVector(int(h), ops[0].n) for h in out if h]
            after = gpu.pool_stats()
            assert len(kept) == bin(mask).count("1")
            assert after.n_kernel_launches == before.n_kernel_launches + 1 and after.n_live_vectors == before.n_live_vectors + len(kept)
            del kept
        # the call computed BOTH pending operands: reading them afterwards launches nothing more …
        before = gpu.pool_stats().n_kernel_launches
        price.to_float32(); forward.to_float32()
        assert gpu.pool_stats().n_kernel_launches == before
        # … and it did so in ONE flush: as many launches as one flush of the same two chains, plus the call's own
        price2 = stored.v1s1("MULT_S", 0.05).v1s1("ADD_S", 4.0); forward2 = stored.v1s1("MULT_S", 0.1).v1s1("ADD_S", 90.0)
        before = gpu.pool_stats().n_kernel_launches
        gpu.flush()
        one_flush = gpu.pool_stats().n_kernel_launches - before
        price3 = stored.v1s1("MULT_S", 0.05).v1s1("ADD_S", 4.0); price3.to_float32()
        forward3 = stored.v1s1("MULT_S", 0.1).v1s1("ADD_S", 90.0)
        before = gpu.pool_stats().n_kernel_launches
        forward3.to_float32()
        print(f"launches: the call {flushed}, one flush of both chains {one_flush}, a flush of one chain {gpu.pool_stats().n_kernel_launches - before}")
        assert one_flush >= 1 and flushed == one_flush + 1
        del price2, forward2
    finally:
        gpu.set_fusion(prev)


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32) * np.float32(0.01) + np.float32(60.0))
        ys = [base.v1s1("MULT_S", 0.1 * k) for k in range(1, 4)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for y in ys:
            try:
                y.to_float32()
                read_error = None
            except gpu.FmhipError as e:
                read_error = e.code
            call = lambda: gpu.implied_volatility("bachelier", gpu.RandomVariableHip(0.0, y), gpu.RandomVariableHip(0.0, base), 1.0, 100.0)
            if read_error is None:
                call()
            else:
                with pytest.raises(gpu.FmhipError) as info: call()
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
res = {}
launches = 0
for model in ("black_scholes", "bachelier"):
    P, F, U = (fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(data[model + k])) for k in ("P", "F", "U"))
    before = fm.pool_stats().n_kernel_launches
    all_three = fm.implied_volatility(model, P, F, 1.5, 100.0, U, ("volatility", "d_price", "d_forward"))
    launches += fm.pool_stats().n_kernel_launches - before
    mixed = fm.implied_volatility(model, P, 104.5, 1.5, 100.0, U, ("d_forward", "volatility"))
    res.update({model + "all%%d" %% f: o.realizations.to_float32() for f, o in enumerate(all_three)})
    res.update({model + "mixed%%d" %% f: o.realizations.to_float32() for f, o in enumerate(mixed)})
    res[model + "P"] = P.realizations.to_float32()
np.savez(out_path, **res)
print("LAUNCHES", launches)
fm.shutdown()
'''


@pytest.fixture(scope="module")
def child_case(gpu, tmp_path_factory):
    want, data = {}, {}
    for model in (0, 1):
        name = NAMES[model]
        P, F, U = operands(gpu, 100_003, model, 9)
        data.update({name + "P": P, name + "F": F, name + "U": U})
        want.update({name + f"all{f}": o for f, o in enumerate(gpu.implied_volatility_host(name, P, F, 1.5, 100.0, U, ("volatility", "d_price", "d_forward")))})
        want.update({name + f"mixed{f}": o for f, o in enumerate(gpu.implied_volatility_host(name, P, 104.5, 1.5, 100.0, U, ("d_forward", "volatility")))})
        want[name + "P"] = P
    folder = tmp_path_factory.mktemp("implied_children")
    np.savez(folder / "in.npz", **data)
    (folder / "child.py").write_text(_CHILD % {"root": ROOT})
    return folder, want


@pytest.mark.parametrize("mode", ["device", "knob_off", "devices_two"])
def test_the_knob_and_a_device_list_give_the_same_bits(child_case, mode):
    """A fresh process on the device, one with FMHIP_DEVICE_ANALYTIC=0 (download, the definition on one core, upload: no launch of the
    kernel) and one behind fm.init_devices([0, 0]) (every shard its block): the bits of the definition, all three."""
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
def test_the_mirrors_keep_the_time_and_take_a_put_and_a_strike_per_path(gpu):
    n = 4 * TILE + 5
    P, F, U = operands(gpu, n, 0, 4)
    vol, slope = gpu.implied_volatility("black_scholes", gpu.RandomVariableHip(0.5, P), gpu.RandomVariableHip(2.0, F), 1.5, 100.0, gpu.RandomVariableHip(1.0, U), ("volatility", "d_price"))
    assert vol.getFiltrationTime() == slope.getFiltrationTime() == 2.0      # the operands' maximum
    want = gpu.implied_volatility_host("black_scholes", P, F, 1.5, 100.0, U, ("volatility", "d_price"))
    assert (bits(vol.realizations.to_float32()) == bits(want[0])).all() and (bits(slope.realizations.to_float32()) == bits(want[1])).all()
    mixed = gpu.bachelier_implied_volatility(gpu.RandomVariableHip(0.5, P), 104.5, 1.5, 100.0, gpu.RandomVariableHip(3.0, 0.9))      # a deterministic operand is a scalar
    assert mixed.getFiltrationTime() == 3.0 and (bits(mixed.realizations.to_float32()) == bits(gpu.implied_volatility_host("bachelier", P, 104.5, 1.5, 100.0, 0.9)[0])).all()
    # a put by parity and a strike per path: the recorded conversions, then the entry point — the bits of the same steps on the host
    rng = np.random.default_rng(6)
    F = rng.uniform(80.0, 125.0, n).astype(np.float32); Ks = rng.uniform(90.0, 110.0, n).astype(np.float32); sigma = rng.uniform(0.1, 0.6, n).astype(np.float32)
    f, k = gpu.RandomVariableHip(0.0, F), gpu.RandomVariableHip(0.0, Ks)
    call = gpu.option_formula("black_scholes", f.div(k), gpu.RandomVariableHip(0.0, sigma), 1.5, 1.0)[0].mult(k)
    put = call.sub(f.sub(k))
    back = gpu.black_scholes_implied_volatility(put, f, 1.5, k, put=True).realizations.to_float32()
    assert np.allclose(back, sigma, rtol=2e-2) and np.median(np.abs(back - sigma) / sigma) < 1e-5
    there = gpu.convert_volatility("black_scholes", "bachelier", f, gpu.RandomVariableHip(0.0, sigma), 1.5, 100.0)
    again = gpu.convert_volatility("bachelier", "black_scholes", f, there, 1.5, 100.0).realizations.to_float32()
    assert np.median(np.abs(again - sigma) / sigma) < 1e-5


def test_aad_value_and_partials_come_from_one_launch(gpu):
    n = 2 * TILE + 9
    rng = np.random.default_rng(5)
    F = rng.uniform(80.0, 125.0, n).astype(np.float32); sigma = rng.uniform(0.1, 0.6, n).astype(np.float32); U = rng.uniform(0.5, 1.5, n).astype(np.float32)
    P = gpu.option_formula_host("black_scholes", F, sigma, 1.5, 100.0, 1.0)[0]
    factory = gpu.RandomVariableDifferentiableAADFactory(gpu.RandomVariableHipFactory())
    p, f, u = (factory.createRandomVariable(0.0, a) for a in (P, F, U))
    for v in (p, f, u): v.getValues().realizations.to_float32()              # stored: nothing of them is pending
    before = gpu.pool_stats().n_kernel_launches
    vol, = gpu.implied_volatility("black_scholes", p, f, 1.5, 100.0, 1.0)
    assert gpu.pool_stats().n_kernel_launches == before + 1                  # value AND both partials
    s1, dp, df = gpu.implied_volatility_host("black_scholes", P, F, 1.5, 100.0, 1.0, ("volatility", "d_price", "d_forward"))
    assert (bits(vol.getValues().realizations.to_float32()) == bits(s1)).all()
    gradient = vol.average().getGradient()
    assert (bits(gradient[p.getID()].getRealizations()) == bits(dp)).all() and (bits(gradient[f.getID()].getRealizations()) == bits(df)).all()
    # with a payoff unit: c = price/unit is a recorded division, and ∂σ/∂N = −(price/N)·∂σ/∂price follows from it
    scaled = p.mult(u)
    gradient = gpu.implied_volatility("black_scholes", scaled, f, 1.5, 100.0, u)[0].average().getGradient()
    assert np.allclose(gradient[u.getID()].getRealizations(), 0.0, atol=2e-6 * np.abs(dp * P).max())      # price = c·N: sigma does not depend on N
    assert np.allclose(gradient[p.getID()].getRealizations(), dp, rtol=1e-4)


# ---------------------------------------------------------------- the driver
_DRIVER = r'''
import importlib, json, sys
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
case = json.loads(sys.argv[1])
fm.init(0)
bm_outer = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, case["steps"], case["dt"]), 2, case["outer"], case["seed_outer"])
bm_inner = fm.BrownianMotionHip(fm.TimeDiscretization(case["time"], case["steps"], case["dt"]), 2, case["outer"] * case["inner"], case["seed_inner"])
rows = mc.forward_implied_volatility_mc(bm_outer, bm_inner, case["inner"], case["initial_value"], case["risk_free_rate"], case["theta"], case["kappa"], case["theta"], case["xi"],
                                        case["rho"], case["time"], case["maturity"], moneyness=tuple(case["moneyness"]), quantiles=tuple(case["quantiles"]))
print("ROWS", json.dumps(rows))
fm.shutdown()
'''
KNOBS_ON = {"FMHIP_DEVICE_ANALYTIC": "1", "FMHIP_DEVICE_NESTED": "1"}
KNOBS_OFF = {"FMHIP_DEVICE_ANALYTIC": "0", "FMHIP_DEVICE_NESTED": "0"}


def run_driver(tmp_path, case, knobs):
    """montecarlo.forward_implied_volatility_mc in a fresh process (the knobs are its environment): the line of its rows, and the rows."""
    script = tmp_path / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT})
    r = subprocess.run([sys.executable, str(script), json.dumps(case)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **knobs))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1]
    return line, json.loads(line[5:])


@pytest.mark.parametrize("seeds", DRIVER_CASE["seeds"])
def test_the_forward_smile_driver_without_vol_of_vol_finds_the_volatility_it_was_given(gpu, oracle, tmp_path, seeds):
    """The driver ITSELF at 256 outer × 64 inner paths with xi = 0 and v0 = theta, with the knobs off and with them on: at moneyness 1 the mean
    future implied volatility is within 5 of its own standard errors of √theta and the not-invertible share is exactly 0 (a zero price at the
    forward at-the-money strike needs all 64 payoffs to be zero); both runs give the same numbers bit for bit; and every number of every
    moneyness — mean, standard error, share, quantiles — is the one of the numpy restatement of the driver's docstring on the same draws
    (tests/test_implied_volatility_cpu.py: other exp and sqrt than the kernels', so 1e-4, a twentieth of a standard error; the maturity
    T − t, the strike m·S_t·e^{r(T − t)}, the share and the quantile levels each move a number by far more)."""
    case = {k: v for k, v in DRIVER_CASE.items() if k != "seeds"}
    case.update(xi=0.0, seed_outer=seeds[0], seed_inner=seeds[1])
    off_line, off = run_driver(tmp_path, case, KNOBS_OFF)
    on_line, on = run_driver(tmp_path, case, KNOBS_ON)
    print(off_line)
    want = restated_forward_smile(gpu, oracle, *seeds)
    for rows in (off, on):
        at_the_money = rows[1]
        assert at_the_money["moneyness"] == 1.0 and at_the_money["not_invertible"] == 0.0
        assert abs(at_the_money["mean"] - math.sqrt(case["theta"])) <= 5 * at_the_money["standard_error"]
        for row, w in zip(rows, want):
            assert row["moneyness"] == w["moneyness"] and abs(row["not_invertible"] - w["not_invertible"]) <= 1.0 / case["outer"]
            same_paths = row["not_invertible"] == w["not_invertible"]           # (a price within an fp32 rounding of the intrinsic value may fall on either side)
            assert same_paths or row["moneyness"] != 1.0
            tolerance = 1e-4 if same_paths else 2e-3
            assert abs(row["mean"] - w["mean"]) <= tolerance and abs(row["standard_error"] - w["standard_error"]) <= tolerance, (row, w)
            if same_paths: assert np.allclose(row["quantiles"], w["quantiles"], rtol=0, atol=1e-4), (row, w)
    assert on_line == off_line


def test_the_forward_smile_driver_equals_its_run_with_the_knobs_off(gpu, tmp_path):
    """montecarlo.forward_implied_volatility_mc at 1024 outer × 256 inner paths with xi > 0, once on the device and once with
    FMHIP_DEVICE_ANALYTIC=0 and FMHIP_DEVICE_NESTED=0: the same numbers, bit for bit (the host definitions are the device's)."""
    case = {k: v for k, v in DRIVER_CASE.items() if k != "seeds"}
    case.update(outer=1024, inner=256, xi=0.5, seed_outer=4711, seed_inner=1147)
    on_line, rows = run_driver(tmp_path, case, KNOBS_ON)
    off_line, _ = run_driver(tmp_path, case, KNOBS_OFF)
    print(on_line)
    assert on_line == off_line
    assert [row["moneyness"] for row in rows] == [0.9, 1.0, 1.1]
    for row in rows:
        assert 0.1 < row["mean"] < 0.3 and 0.0 < row["standard_error"] < 0.01 and row["quantiles"] == sorted(row["quantiles"], reverse=True) and 0.0 <= row["not_invertible"] < 0.05
    assert rows[0]["mean"] > rows[2]["mean"]                                 # rho < 0: the forward smile is a skew
