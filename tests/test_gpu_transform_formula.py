"""Transform option values per path on the device (include/fmhip.h: fmhip_transform_option; csrc/transform_kernel.hip) on a
real MI355X.  Every check of the kernel is an EQUALITY of bits with the host definition (fmhip_transform_option_host): sizes around the
kernel's group, tile and the wrap of its grid-stride loop (read from csrc/transform_kernel.h), 0, 1 and 2 states, tables of 1, 2, 63, 64,
65 and 256 nodes (256 up to four tiles: the host twin runs on one core), every mask the state count allows, every combination of vector
and scalar operands, the edge rows of tests/test_transform_formula_cpu.py planted in the first, a middle and the last group; operands are
only read; pending operands computed in one flush and one launch for the call, exactly the outputs in the pool, given-up values, the
FMHIP_DEVICE_ANALYTIC=0 path and a device list of two shards in child processes, the mirrors with a put and a strike per path, the AAD
triple from one launch, and the forward-smile driver against its numpy restatement on the same draws.  No test asks the device for anything
out of range: bad arguments are refused on the host before a launch."""
import ctypes as C
import itertools
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_transform_formula_cpu import DRIVER_CASE, QUIET_NAN, bits, edge_rows, make_table, operands, restated_forward_smile_transform, transform_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PD = C.POINTER(C.c_double)


def header_constants():
    text = open(os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "csrc", "transform_kernel.h")).read()
    env = {}
    for name, expr in re.findall(r"constexpr int (FM_TRANSFORM_\w+) = ([^;,]+)[;,]", text):
        try: env[name] = int(eval(expr, {"__builtins__": {}}, env))
        except Exception: pass                                                 # (one that is written in terms of the definition's header)
    return env


K_ = header_constants()
BLOCK, TILE, MAX_BLOCKS = K_["FM_TRANSFORM_BLOCK"], K_["FM_TRANSFORM_TILE"], K_["FM_TRANSFORM_MAX_BLOCKS"]
assert TILE == BLOCK * 4                                                     # a lane takes one 16-byte group per iteration
WRAP = MAX_BLOCKS * TILE + 1                                                 # the smallest n whose grid-stride loop runs a second time in some lane
assert -(-WRAP // TILE) > MAX_BLOCKS and -(-(WRAP - 1) // TILE) == MAX_BLOCKS and WRAP + 3 < 4_000_000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, WRAP + 3, 100_003]
NODE_COUNTS = [1, 2, 63, 64, 65, 256]
SCALARS = (104.5, 0.9, 0.03, 0.015)                                          # forward, payoff unit, V_0, V_1


def device_transform(gpu, table, S, ops, K, mask):
    """fmhip_transform_option through ctypes: ops = (forward, payoff unit, V_0, V_1), DeviceVectors or floats; the columns in bit order."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    handles = [o.handle if isinstance(o, gpu.DeviceVector) else 0 for o in ops]
    scalars = [0.0 if isinstance(o, gpu.DeviceVector) else float(o) for o in ops]
    n = next(o.n for o in ops if isinstance(o, gpu.DeviceVector))
    states = (C.c_int64 * 2)(*handles[2:4]); state_scalars = (C.c_double * 2)(*scalars[2:4])
    out = (C.c_int64 * bin(mask).count("1"))()
    gpu._native.check(gpu.lib().fmhip_transform_option(table.ctypes.data_as(PD), table.shape[0], S, handles[0], scalars[0], states if S else None, state_scalars if S else None,
                                                       handles[1], scalars[1], float(K), mask, out))
    return [gpu.DeviceVector(int(h), n).to_float32() for h in out]


def check(gpu, table, S, arrays, use_vector, K, mask):
    use_vector = tuple(use and k < 2 + S for k, use in enumerate(use_vector))
    vectors = [gpu.DeviceVector.from_host(a) if use else None for a, use in zip(arrays, use_vector)]
    device_ops = [v if use else s for v, use, s in zip(vectors, use_vector, SCALARS)]
    host_ops = [a if use else s for a, use, s in zip(arrays, use_vector, SCALARS)]
    got, want = device_transform(gpu, table, S, device_ops, K, mask), transform_host(gpu, table, S, host_ops, K, mask)
    assert len(got) == len(want) == bin(mask).count("1")
    for f, (g, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero(bits(g) != bits(w))
        assert differ.size == 0, (table.shape, S, use_vector, mask, f, differ[:5], [a[differ[:5]] for a in arrays], g[differ[:5]], w[differ[:5]])
    for v, a in zip(vectors, arrays):
        if v is not None: assert (bits(v.to_float32()) == bits(a)).all()      # the pass only reads its operands


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("S", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_every_size_equals_the_definition(gpu, S, n):
    J = 2 if n > 4 * TILE else NODE_COUNTS[(n + S) % len(NODE_COUNTS)]        # the host twin runs J·n nodes on one core
    arrays = operands(n, S, n + S)
    check(gpu, make_table(J, S), S, arrays, (True, True, True, True), 100.0, 7 if S else 3)
    if n <= 4 * TILE: check(gpu, make_table(64, S), S, arrays, (True, n % 2 == 0, S >= 1, False), 100.0, 1 + n % (7 if S else 3))


@pytest.mark.parametrize("S", [0, 1, 2])
@pytest.mark.parametrize("J", NODE_COUNTS)
def test_every_node_count_every_mask_and_every_combination_of_vector_and_scalar_operands(gpu, S, J):
    n = (3 * TILE + 7) if J < 256 else TILE + 7
    arrays = operands(n, S, 17 + J)
    table = make_table(J, S)
    masks = range(1, 8) if S else range(1, 4)
    combos = [c for c in itertools.product([True, False], repeat=2 + S) if any(c)]
    if J in (64, 65):
        for use_vector in combos:
            for mask in masks: check(gpu, table, S, arrays, use_vector + (False,) * (2 - S), 100.0, mask)
    else:
        for i, use_vector in enumerate(combos): check(gpu, table, S, arrays, use_vector + (False,) * (2 - S), 100.0, list(masks)[i % len(masks)])
    check(gpu, table, S, arrays, (True, True, True, True), 0.0, 3)             # a strike that is no strike: the limit everywhere
    check(gpu, table, S, arrays, (True, True, True, True), float("inf"), 1)


def test_a_model_table_equals_the_definition(gpu):
    nodes = gpu.heston_transform_nodes(1.5, 0.04, 0.5, -0.7, 0.5)
    arrays = operands(2 * TILE + 3, 1, 2)
    check(gpu, nodes.table, 1, arrays, (True, True, True, False), 100.0, 7)


@pytest.mark.parametrize("S", [0, 1, 2])
def test_the_edge_rows_are_where_they_were_planted(gpu, S):
    """The planted elements answer what the contract states, on the device: the equality above compares with a host that could share a mistake."""
    n = 100_003
    arrays = operands(n, S, 3)
    got = device_transform(gpu, make_table(2, S), S, [gpu.DeviceVector.from_host(a) if k < 2 + S else 0.0 for k, a in enumerate(arrays)], 100.0, 7 if S else 3)
    rows = edge_rows(S)
    for start in (0, (n // 2) // 4 * 4, n - len(rows)):
        for i, (f, u, _, _, what) in enumerate(rows):
            p = start + i
            column = [bits(g[p:p + 1])[0] for g in got]
            if what == "nan": assert all(b == QUIET_NAN for b in column)
            elif what == "limit": assert got[0][p] == u * max(f - 100.0, 0.0) and got[1][p] == (u if f > 100.0 else 0.0) and (S == 0 or got[2][p] == 0.0)
            elif what == "live": assert all(np.isfinite(g[p]) for g in got)
            else: assert not np.isfinite(got[0][p]) and all(b == QUIET_NAN for g, b in zip(got, column) if np.isnan(g[p]))


def test_refused_on_the_host_before_anything_runs(gpu):
    v = gpu.DeviceVector.from_host(np.full(8, 100.0, dtype=np.float32)); w = gpu.DeviceVector.from_host(np.ones(9, dtype=np.float32))
    table = make_table(8, 1)
    tp = table.ctypes.data_as(PD)
    bad = table.copy(); bad[2, 1] = np.inf
    before = gpu.pool_stats()
    out = (C.c_int64 * 3)()
    lib, E = gpu.lib(), gpu._native
    none, one_state = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(w.handle, 0)
    scalars = (C.c_double * 2)(0.04, 0.0)
    assert lib.fmhip_transform_option(tp, 8, 1, 0, 100.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT          # no vector
    assert lib.fmhip_transform_option(tp, 0, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 257, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 3, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, -1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 3, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 8, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 0, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(make_table(8, 0).ctypes.data_as(PD), 8, 0, v.handle, 0.0, None, None, 0, 1.0, 100.0, 4, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(None, 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, None, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, none, None, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, None) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(bad.ctypes.data_as(PD), 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, none, scalars, 0, 1.0, float("nan"), 7, out) == E.ERR_INVALID_ARGUMENT
    assert lib.fmhip_transform_option(tp, 8, 1, v.handle, 0.0, one_state, scalars, 0, 1.0, 100.0, 7, out) == E.ERR_SIZE_MISMATCH
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors and list(out) == [0] * 3


def test_pending_operands_are_computed_in_one_flush_and_the_call_is_one_launch(gpu):
    prev = gpu.set_fusion(True)
    try:
        rng = np.random.default_rng(1)
        base = rng.uniform(60.0, 140.0, TILE + 77).astype(np.float32)
        stored = gpu.DeviceVector.from_host(base)
        table = make_table(64, 1)
        forward = stored.v1s1("MULT_S", 0.1).v1s1("ADD_S", 90.0); variance = stored.v1s1("MULT_S", 0.001).v1s1("ADD_S", 0.01)      # nothing has run yet
        before = gpu.pool_stats().n_kernel_launches
        got = device_transform(gpu, table, 1, [forward, 0.9, variance, 0.0], 100.0, 7)
        flushed = gpu.pool_stats().n_kernel_launches - before
        want = transform_host(gpu, table, 1, (forward.to_float32(), 0.9, variance.to_float32(), 0.0), 100.0, 7)
        assert all((bits(g) == bits(w)).all() for g, w in zip(got, want)) and np.isfinite(want[0]).all()
        # stored operands: exactly one launch, exactly the outputs in the pool
        ops = [gpu.DeviceVector.from_host(a) for a in operands(5 * TILE + 3, 1, 5)[:3]]
        tp = table.ctypes.data_as(PD)
        for mask in range(1, 8):
            before = gpu.pool_stats()
            out = (C.c_int64 * 3)()
            gpu._native.check(gpu.lib().fmhip_transform_option(tp, 64, 1, ops[0].handle, 0.0, (C.c_int64 * 1)(ops[2].handle), (C.c_double * 1)(0.0), ops[1].handle, 0.0, 100.0, mask, out))
            kept = [gpu.DeviceVector(int(h), ops[0].n) for h in out if h]
            after = gpu.pool_stats()
            assert len(kept) == bin(mask).count("1")
            assert after.n_kernel_launches == before.n_kernel_launches + 1 and after.n_live_vectors == before.n_live_vectors + len(kept)
            del kept
        # the call computed BOTH pending operands: reading them afterwards launches nothing more …
        before = gpu.pool_stats().n_kernel_launches
        forward.to_float32(); variance.to_float32()
        assert gpu.pool_stats().n_kernel_launches == before
        # … and it did so in ONE flush: as many launches as one flush of the same two chains, plus the call's own
        forward2 = stored.v1s1("MULT_S", 0.1).v1s1("ADD_S", 90.0); variance2 = stored.v1s1("MULT_S", 0.001).v1s1("ADD_S", 0.01)
        before = gpu.pool_stats().n_kernel_launches
        gpu.flush()
        one_flush = gpu.pool_stats().n_kernel_launches - before
        print(f"launches: the call {flushed}, one flush of both chains {one_flush}")
        assert one_flush >= 1 and flushed == one_flush + 1
        del forward2, variance2
    finally:
        gpu.set_fusion(prev)


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32) * np.float32(0.01) + np.float32(60.0))
        ys = [base.v1s1("MULT_S", 0.001 * k) for k in range(1, 4)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        nodes = gpu.TransformNodes(make_table(8, 1), 1)
        for y in ys:
            try:
                y.to_float32()
                read_error = None
            except gpu.FmhipError as e:
                read_error = e.code
            call = lambda: gpu.transform_option_value(nodes, gpu.RandomVariableHip(0.0, base), (gpu.RandomVariableHip(0.0, y),), 100.0)
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
for S in (0, 1, 2):
    nodes = fm.TransformNodes(data["table%%d" %% S], S)
    F, U, A, B = (fm.RandomVariableHip(0.0, fm.DeviceVector.from_host(data["S%%d%%s" %% (S, k)])) for k in "FUAB")
    states = (A, B)[:S]
    names = ("value", "delta", "state_delta")[:3 if S else 2]
    before = fm.pool_stats().n_kernel_launches
    every = fm.transform_option_value(nodes, F, states, 100.0, U, names)
    launches += fm.pool_stats().n_kernel_launches - before
    mixed = fm.transform_option_value(nodes, F, (0.03, B)[:S], 100.0, 0.9, ("delta", "value"))
    res.update({"S%%dall%%d" %% (S, f): o.realizations.to_float32() for f, o in enumerate(every)})
    res.update({"S%%dmixed%%d" %% (S, f): o.realizations.to_float32() for f, o in enumerate(mixed)})
    res["S%%dF" %% S] = F.realizations.to_float32()
np.savez(out_path, **res)
print("LAUNCHES", launches)
fm.shutdown()
'''


@pytest.fixture(scope="module")
def child_case(gpu, tmp_path_factory):
    want, data = {}, {}
    for S in (0, 1, 2):
        table = make_table(16, S)
        nodes = gpu.TransformNodes(table, S)
        F, U, A, B = operands(100_003, S, 9 + S)
        data.update({f"table{S}": table, f"S{S}F": F, f"S{S}U": U, f"S{S}A": A, f"S{S}B": B})
        names = ("value", "delta", "state_delta")[:3 if S else 2]
        want.update({f"S{S}all{f}": o for f, o in enumerate(gpu.transform_option_host(nodes, F, (A, B)[:S], 100.0, U, names))})
        want.update({f"S{S}mixed{f}": o for f, o in enumerate(gpu.transform_option_host(nodes, F, (0.03, B)[:S], 100.0, 0.9, ("delta", "value")))})
        want[f"S{S}F"] = F
    folder = tmp_path_factory.mktemp("transform_children")
    np.savez(folder / "in.npz", **data)
    (folder / "child.py").write_text(_CHILD % {"root": ROOT})
    return folder, want


@pytest.mark.parametrize("mode", ["device", "knob_off", "devices_two"])
def test_the_knob_and_a_device_list_give_the_same_bits(child_case, mode):
    """A fresh process on the device, one with FMHIP_DEVICE_ANALYTIC=0 (download, the definition on one core, upload: no launch of the
    kernel) and one behind fm.init_devices([0, 0]) (every shard its block): the bits of the definition."""
    folder, want = child_case
    out_path = folder / (mode + ".npz")
    r = subprocess.run([sys.executable, str(folder / "child.py"), mode, str(out_path), str(folder / "in.npz")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FMHIP_DEVICE_ANALYTIC="0" if mode == "knob_off" else "1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    launches = int([line for line in r.stdout.splitlines() if line.startswith("LAUNCHES ")][-1].split()[1])
    res = dict(np.load(out_path))
    for name, w in want.items(): assert (bits(res[name]) == bits(w)).all(), (mode, name)
    if mode == "device": assert launches == 3                                # one per call
    if mode == "knob_off": assert launches == 0


# ---------------------------------------------------------------- the mirrors
def test_the_mirrors_keep_the_time_and_take_a_put_and_a_strike_per_path(gpu):
    n = 4 * TILE + 5
    nodes = gpu.heston_transform_nodes(1.5, 0.04, 0.5, -0.7, 1.0, n_nodes=64)
    rng = np.random.default_rng(4)
    F = rng.uniform(60.0, 160.0, n).astype(np.float32); V = rng.uniform(0.0, 0.3, n).astype(np.float32); U = rng.uniform(0.5, 1.5, n).astype(np.float32)
    value, slope = gpu.transform_option_value(nodes, gpu.RandomVariableHip(0.5, F), gpu.RandomVariableHip(2.0, V), 100.0, gpu.RandomVariableHip(1.0, U), ("value", "state_delta"))
    assert value.getFiltrationTime() == slope.getFiltrationTime() == 2.0    # the operands' maximum
    want = gpu.transform_option_host(nodes, F, (V,), 100.0, U, ("value", "state_delta"))
    assert (bits(value.realizations.to_float32()) == bits(want[0])).all() and (bits(slope.realizations.to_float32()) == bits(want[1])).all()
    mixed, = gpu.heston_option_value(gpu.RandomVariableHip(0.5, F), gpu.RandomVariableHip(3.0, 0.05), 1.0, 100.0, 1.5, 0.04, 0.5, -0.7, nodes=nodes)      # a deterministic operand is a scalar
    assert mixed.getFiltrationTime() == 3.0 and (bits(mixed.realizations.to_float32()) == bits(gpu.transform_option_host(nodes, F, (0.05,), 100.0)[0])).all()
    # a put by parity and a strike per path: the recorded conversions around the entry point, against the same steps on the host (the
    # engine's division F/K may differ from numpy's in the last place: a value moves by delta·K times that)
    Ks = rng.uniform(80.0, 125.0, n).astype(np.float32)
    f, v, k = gpu.RandomVariableHip(0.0, F), gpu.RandomVariableHip(0.0, V), gpu.RandomVariableHip(0.0, Ks)
    call, delta = gpu.transform_option_value(nodes, f, v, k, 1.0, ("value", "delta"))
    unit = gpu.transform_option_host(nodes, (F / Ks).astype(np.float32), (V,), 1.0, 1.0, ("value", "delta"))
    assert np.allclose(call.realizations.to_float32(), unit[0] * Ks, rtol=1e-6, atol=3e-5) and np.allclose(delta.realizations.to_float32(), unit[1], rtol=0, atol=2e-6)
    put, put_delta = gpu.transform_option_value(nodes, f, v, k, 1.0, ("value", "delta"), put=True)
    assert np.allclose(put.realizations.to_float32(), unit[0] * Ks - (F - Ks), rtol=1e-6, atol=3e-5) and np.allclose(put_delta.realizations.to_float32(), unit[1] - np.float32(1.0), rtol=0, atol=2e-6)
    assert (put.realizations.to_float32() > -1e-3).all() and (put_delta.realizations.to_float32() <= 0.0).all()
    # a put at a scalar strike is parity on the definition's bits
    put_100, = gpu.transform_option_value(nodes, f, v, 100.0, 1.0, ("value",), put=True)
    assert (bits(put_100.realizations.to_float32()) == bits(gpu.transform_option_host(nodes, F, (V,), 100.0)[0] - (F - np.float32(100.0)))).all()
    # Bates' mirror: jumps make every call worth more
    bates, = gpu.bates_option_value(f, v, 1.0, 100.0, 1.5, 0.04, 0.5, -0.7, 0.4, -0.1, 0.2)
    assert (bates.realizations.to_float32() >= want[0] / U - 1e-4).all()


def test_aad_value_and_partials_come_from_one_launch(gpu):
    n = 2 * TILE + 9
    nodes = gpu.heston_transform_nodes(1.5, 0.04, 0.5, -0.7, 1.0, n_nodes=64)
    rng = np.random.default_rng(5)
    F = rng.uniform(80.0, 125.0, n).astype(np.float32); V = rng.uniform(0.01, 0.3, n).astype(np.float32); U = rng.uniform(0.5, 1.5, n).astype(np.float32)
    factory = gpu.RandomVariableDifferentiableAADFactory(gpu.RandomVariableHipFactory())
    f, v, u = (factory.createRandomVariable(0.0, a) for a in (F, V, U))
    for x in (f, v, u): x.getValues().realizations.to_float32()              # stored: nothing of them is pending
    before = gpu.pool_stats().n_kernel_launches
    value, = gpu.transform_option_value(nodes, f, v, 100.0)
    assert gpu.pool_stats().n_kernel_launches == before + 1                  # value AND both partials
    want, delta, slope = gpu.transform_option_host(nodes, F, (V,), 100.0, 1.0, ("value", "delta", "state_delta"))
    assert (bits(value.getValues().realizations.to_float32()) == bits(want)).all()
    gradient = value.average().getGradient()
    assert (bits(gradient[f.getID()].getRealizations()) == bits(delta)).all() and (bits(gradient[v.getID()].getRealizations()) == bits(slope)).all()
    # with a payoff unit: the value is the unit value times it, by a recorded product
    gradient = gpu.transform_option_value(nodes, f, v, 100.0, u)[0].average().getGradient()
    assert np.allclose(gradient[u.getID()].getRealizations(), want, rtol=1e-6) and np.allclose(gradient[f.getID()].getRealizations(), delta * U, rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------- the driver
_DRIVER = r'''
import importlib, json, sys
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
case = json.loads(sys.argv[1])
fm.init(0)
bm_outer = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, case["steps"], case["dt"]), 2, case["outer"], case["seed_outer"])
rows = mc.forward_implied_volatility_transform_mc(bm_outer, case["initial_value"], case["risk_free_rate"], case["v0"], case["kappa"], case["theta"], case["xi"], case["rho"],
                                                  case["time"], case["maturity"], moneyness=tuple(case["moneyness"]), quantiles=tuple(case["quantiles"]))
print("ROWS", json.dumps(rows))
fm.shutdown()
'''


def test_the_forward_smile_driver_against_its_numpy_restatement(gpu, oracle, tmp_path):
    """montecarlo.forward_implied_volatility_transform_mc at 4096 outer paths in a fresh process, with the knob on and off: the same numbers bit
    for bit, and each — mean, standard error, share — the one of the numpy restatement on the same draws (other exp and sqrt than the
    kernels': 1e-4, a twentieth of a standard error).  No inner noise: every path's price is invertible."""
    script = tmp_path / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT})
    lines = {}
    for knob in ("1", "0"):
        r = subprocess.run([sys.executable, str(script), json.dumps(DRIVER_CASE)], capture_output=True, text=True, timeout=300, env=dict(os.environ, FMHIP_DEVICE_ANALYTIC=knob))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines[knob] = [l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1]
    print(lines["1"])
    assert lines["1"] == lines["0"]
    rows = json.loads(lines["1"][5:])
    want = restated_forward_smile_transform(gpu, oracle, DRIVER_CASE)
    for row, w in zip(rows, want):
        assert row["moneyness"] == w["moneyness"] and row["not_invertible"] == w["not_invertible"] == 0.0
        assert abs(row["mean"] - w["mean"]) <= 1e-4 and abs(row["standard_error"] - w["standard_error"]) <= 1e-4, (row, w)
        assert 0.1 < row["mean"] < 0.3 and 0.0 < row["standard_error"] < 0.01 and row["quantiles"] == sorted(row["quantiles"], reverse=True)
    assert rows[0]["mean"] > rows[2]["mean"]                                 # rho < 0: the forward smile is a skew
