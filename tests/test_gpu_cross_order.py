"""Order statistics across vectors on the device (include/fmhip.h: fmhip_cross_order_statistics, fmhip_cross_select;
csrc/cross_order_kernel.hip) on a real MI355X: values and indices EQUAL the host definition's bit for bit for every K of
the issue's list — every padded network size with its neighbours — at sizes around a wave, past a group of four and past the grid's cap;
an output's bits do not depend on the other selectors or the mask; the knob-off path, a device list of two shards and thread engines give
the same bits; max_across equals the floor chain; pending operands; refusals on the host; and the max-call driver with ordered states.

Every test prints the figures it asserts on before it asserts (run with -s).  No test asks the device for anything out of range: bad
arguments are refused on the host before a launch, and an index that names no slot loads nothing."""
import contextlib
import ctypes as C
import os
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_cross_order_cpu import KS, NS, QUIET_NAN, bits, cross_data, some_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = NS + (100003,)


@contextlib.contextmanager
def knob_off():
    prev = os.environ.get("FMHIP_DEVICE_CROSS_ORDER")
    os.environ["FMHIP_DEVICE_CROSS_ORDER"] = "0"
    try:
        yield
    finally:
        if prev is None: del os.environ["FMHIP_DEVICE_CROSS_ORDER"]
        else: os.environ["FMHIP_DEVICE_CROSS_ORDER"] = prev


def upload(gpu, arrays):
    """One DeviceVector per distinct array: the same array in two slots is the same handle in two slots."""
    made = {}
    return [made.setdefault(id(a), gpu.DeviceVector.from_host(a)) for a in arrays]


def device_bits(rvs):
    return [bits(rv.realizations.to_float32()) for rv in rvs]


@pytest.mark.parametrize("k", KS)
def test_values_and_indices_are_the_definitions_bit_for_bit(gpu, k):
    rng = np.random.default_rng(500 + k)
    for n in SIZES:
        arrays = cross_data(k, n, rng)
        vs = upload(gpu, arrays)
        want = [bits(w) for w in gpu.cross_order_statistics_host(arrays, range(k), True, True)]
        got = device_bits(gpu.order_across(vs, range(k), values=True, indices=True))
        assert len(got) == len(want) == 2 * k
        wrong = [(j, int((g != w).sum())) for j, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or (g != w).any()]
        assert not wrong, (k, n, wrong[:4])
        # the bits are unchanged when the call names other ranks or another mask (keys alone, pairs; one selector, duplicates, 32 of them)
        ranks = some_ranks(k)
        only_values, only_slots = device_bits(gpu.order_across(vs, ranks, True, False)), device_bits(gpu.order_across(vs, ranks[::-1], False, True))
        for j, r in enumerate(ranks):
            assert (only_values[j] == want[r]).all(), (k, n, r)
            assert (only_slots[len(ranks) - 1 - j] == want[k + r]).all(), (k, n, r)
        full = device_bits(gpu.order_across(vs, [ranks[0]] * 32, True, True))
        assert all((f == want[ranks[0]]).all() for f in full[:32]) and all((f == want[k + ranks[0]]).all() for f in full[32:])
        # the selection behind the index: value r wherever that value is no NaN, bit for bit the definition's everywhere
        r = k // 2
        slot = gpu.order_across(vs, [r], False, True)[0]
        picked = bits(gpu.select_across(slot, vs).realizations.to_float32())
        assert (picked == bits(gpu.cross_select_host(want[k + r].view(np.float32), arrays))).all()
        assert (picked[want[r] != QUIET_NAN] == want[r][want[r] != QUIET_NAN]).all()
        for v, a in zip(vs, arrays): assert (bits(v.to_float32()) == bits(a)).all()                     # inputs unchanged


def test_cross_select_refuses_every_index_that_names_no_slot(gpu):
    k, n = 5, 1000
    arrays = cross_data(k, n, np.random.default_rng(3))
    vs = upload(gpu, arrays)
    index = np.resize(np.float32([0, 1, 2, 3, 4, -0.0, -1, 5, 0.5, np.nan, np.inf, -np.inf, 4.0000005, 1e30, -1e-30, 31, 32]), n).astype(np.float32)
    got = bits(gpu.select_across(gpu.DeviceVector.from_host(index), vs).realizations.to_float32())
    want = bits(gpu.cross_select_host(index, arrays))
    print("refused indices:", int((want == QUIET_NAN).sum()), "of", n)
    assert (got == want).all()
    valid = np.isin(index, np.float32([0, 1, 2, 3, 4]))
    assert (got[~valid] == QUIET_NAN).all()
    assert (got[valid] == np.stack([bits(a) for a in arrays])[index[valid].astype(int), np.nonzero(valid)[0]]).all()


def test_more_paths_than_the_grid_takes_at_once(gpu):
    """The grid is capped at 2048 workgroups of 256 lanes: four paths a lane up to K = 8, one above."""
    rng = np.random.default_rng(11)
    for k, n in ((3, 2048 * 256 * 4 + 1027), (9, 2048 * 256 + 77)):
        arrays = [rng.standard_normal(n).astype(np.float32) for _ in range(k)]
        arrays[1][::1001] = np.nan
        vs = upload(gpu, arrays)
        want = gpu.cross_order_statistics_host(arrays, [0, k - 1], True, True)
        got = gpu.order_across(vs, [0, k - 1], True, True)
        for g, w in zip(device_bits(got), want): assert (g == bits(w)).all(), (k, n)
        assert (bits(gpu.select_across(got[3], vs).realizations.to_float32()) == bits(gpu.cross_select_host(want[3], arrays))).all()


def test_the_host_switch_gives_identical_results(gpu):
    def everything():
        out = []
        for k in (1, 2, 5, 17):
            arrays = cross_data(k, 2049, np.random.default_rng(k))
            vs = [gpu.RandomVariableHip(1.25, a) for a in arrays]
            rows = gpu.order_across(vs, list(range(k)) * 3, values=True, indices=True)                  # up to 51 selectors: taken in groups
            assert len(rows) == 6 * k and all(rv.getFiltrationTime() == 1.25 for rv in rows)
            rows += gpu.sort_across(vs, descending=True) + [gpu.max_across(vs), gpu.min_across(vs), gpu.median_across(vs), gpu.argmax_across(vs), gpu.argmin_across(vs)]
            rows += [gpu.select_across(gpu.argmax_across(vs), vs), gpu.select_across(gpu.RandomVariableHip(0.0, 0.0), vs)]
            rows += gpu.order_across(vs + [gpu.RandomVariableHip(0.5, 0.25)], [0, k], True, True)       # a deterministic variable among them
            out += device_bits(rows)
        return out
    launches = gpu.pool_stats().n_kernel_launches
    device = everything()
    assert gpu.pool_stats().n_kernel_launches >= launches + 4 * 9
    with knob_off():
        host = everything()
    assert len(device) == len(host)
    for j, (d, h) in enumerate(zip(device, host)): assert d.shape == h.shape and (d == h).all(), j


def test_max_across_equals_the_floor_chain(gpu):
    """On data without NaNs and without zeros of mixed sign the composed chain of floor (the fused op stream's maximum) gives the same bits."""
    rng = np.random.default_rng(12)
    for k in (2, 5, 16):
        arrays = [((10.0 ** rng.uniform(-6.0, 6.0, 4099)) * np.where(rng.random(4099) < 0.5, -1.0, 1.0)).astype(np.float32) for _ in range(k)]
        arrays[k - 1][::7] = arrays[0][::7]
        arrays[0][5], arrays[1][6] = np.inf, -np.inf
        vs = [gpu.RandomVariableHip(0.0, a) for a in arrays]
        chain, low = vs[0], vs[0]
        for v in vs[1:]: chain, low = chain.floor(v), low.cap(v)
        assert (bits(gpu.max_across(vs).realizations.to_float32()) == bits(chain.realizations.to_float32())).all(), k
        assert (bits(gpu.min_across(vs).realizations.to_float32()) == bits(low.realizations.to_float32())).all(), k


def test_pending_operands_and_results_that_outlive_them(gpu):
    n = 4099
    arrays = cross_data(3, n, np.random.default_rng(13))
    arrays[2] = np.random.default_rng(14).standard_normal(n).astype(np.float32)
    prev = gpu.set_fusion(True)
    try:
        stored = [gpu.DeviceVector.from_host(a) for a in arrays]
        pending = [stored[0].v1s1("MULT_S", 2.0), stored[1], stored[2].v1s1("ADD_S", 1.0)]
        got = gpu.order_across(pending, [0, 1, 2], True, True)
        held = [p.to_float32() for p in pending]
        picked = gpu.select_across(got[5].realizations, [stored[2].v1s1("MULT_S", -1.0), stored[0], stored[0].v1s1("ADD_S", 0.5)])
        payload = [(-arrays[2]).astype(np.float32), arrays[0], (arrays[0] + np.float32(0.5)).astype(np.float32)]
        del pending, stored                                                                          # the results stay valid after the operands are released
        want = gpu.cross_order_statistics_host(held, [0, 1, 2], True, True)
        for g, w in zip(device_bits(got), want): assert (g == bits(w)).all()
        assert (bits(picked.realizations.to_float32()) == bits(gpu.cross_select_host(want[5], payload))).all()
    finally:
        gpu.set_fusion(prev)


def test_pool_statistics_show_only_the_outputs_and_one_launch(gpu):
    n = 1 << 16
    vs = [gpu.DeviceVector.from_host(np.random.default_rng(k).random(n, dtype=np.float32)) for k in range(3)]
    gpu.order_across(vs, [0]); vs[0].to_float32()
    before = gpu.pool_stats().bytes_in_use
    probe = gpu.DeviceVector.from_host(np.zeros(n, dtype=np.float32))
    per = gpu.pool_stats().bytes_in_use - before
    del probe
    for call, n_out in ((lambda: gpu.order_across(vs, [0, 2, 2], True, True), 6), (lambda: gpu.order_across(vs, [1], False, True), 1), (lambda: gpu.select_across(vs[0], vs), 1)):
        before = gpu.pool_stats()
        kept = call()
        after = gpu.pool_stats()
        assert after.n_live_vectors - before.n_live_vectors == n_out and after.bytes_in_use - before.bytes_in_use == n_out * per
        assert after.n_kernel_launches == before.n_kernel_launches + 1
        del kept


def test_refusals_are_made_on_the_host(gpu):
    N, lib = gpu._native, gpu.lib()
    n = 1000
    v = gpu.DeviceVector.from_host(np.arange(n, dtype=np.float32))
    other = gpu.DeviceVector.from_host(np.arange(n + 1, dtype=np.float32))
    v.to_float32(); other.to_float32()
    before = gpu.pool_stats()
    outs, h = (C.c_int64 * 64)(), C.c_int64(0)
    vs = lambda *hs: (C.c_int64 * len(hs))(*hs)
    ints = lambda *xs: (C.c_int32 * max(len(xs), 1))(*xs)
    bad, f, g = N.ERR_INVALID_ARGUMENT, lib.fmhip_cross_order_statistics, lib.fmhip_cross_select
    assert f(vs(v.handle), 0, ints(0), 1, 1, outs) == bad
    assert f(vs(*[v.handle] * 33), 33, ints(0), 1, 1, outs) == bad
    assert f(vs(v.handle), 1, ints(0), 0, 1, outs) == bad
    assert f(vs(v.handle), 1, ints(*[0] * 33), 33, 1, outs) == bad
    assert f(vs(v.handle, v.handle), 2, ints(2), 1, 1, outs) == bad
    assert f(vs(v.handle), 1, ints(-1), 1, 1, outs) == bad
    assert f(vs(v.handle), 1, ints(0), 1, 0, outs) == bad
    assert f(vs(v.handle), 1, ints(0), 1, 4, outs) == bad
    assert f(None, 1, ints(0), 1, 1, outs) == bad
    assert f(vs(v.handle), 1, None, 1, 1, outs) == bad
    assert f(vs(v.handle), 1, ints(0), 1, 1, None) == bad
    assert f(vs(v.handle, 0), 2, ints(0), 1, 1, outs) == bad
    assert f(vs(v.handle, other.handle), 2, ints(0), 1, 1, outs) == N.ERR_SIZE_MISMATCH
    assert f(vs(v.handle + 12345), 1, ints(0), 1, 1, outs) == N.ERR_INVALID_HANDLE
    assert g(0, vs(v.handle), 1, C.byref(h)) == bad
    assert g(v.handle, vs(v.handle), 0, C.byref(h)) == bad
    assert g(v.handle, vs(*[v.handle] * 33), 33, C.byref(h)) == bad
    assert g(v.handle, None, 1, C.byref(h)) == bad
    assert g(v.handle, vs(v.handle), 1, None) == bad
    assert g(v.handle, vs(v.handle, 0), 2, C.byref(h)) == bad
    assert g(other.handle, vs(v.handle), 1, C.byref(h)) == N.ERR_SIZE_MISMATCH
    assert g(v.handle, vs(v.handle + 12345), 1, C.byref(h)) == N.ERR_INVALID_HANDLE
    with pytest.raises(ValueError): gpu.order_across([v, other], [0])
    with pytest.raises(ValueError): gpu.max_across([])
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors and after.bytes_in_use == before.bytes_in_use
    assert h.value == 0 and all(x == 0 for x in outs)
    # under an expectation communicator both calls act on this rank's own paths
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        top = gpu.max_across([v, v.v1s1("MULT_S", -1.0)]).realizations.to_float32()
        picked = gpu.select_across(gpu.argmax_across([v.v1s1("MULT_S", -1.0), v]), [v.v1s1("ADD_S", 1.0), v]).realizations.to_float32()
    finally:
        gpu.set_expectation_comm(1, 0, None)
    assert (top == np.arange(n, dtype=np.float32)).all() and (picked == np.arange(n, dtype=np.float32)).all()


# ---------------------------------------------------------------- the fronts: a device list, thread engines
_FRONTS = r'''
import importlib, json, sys, threading
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
from test_cross_order_cpu import cross_data
mode, out_path = sys.argv[1], sys.argv[2]
res = {}
arrays = {k: cross_data(k, 4099, np.random.default_rng(900 + k)) for k in (3, 17)}

def everything(tag, k, vs):
    rows = fm.order_across(vs, range(k), values=True, indices=True)
    for j, rv in enumerate(rows): res["%%s_%%d_%%d" %% (tag, k, j)] = rv.realizations.to_float32()
    res["%%s_%%d_select" %% (tag, k)] = fm.select_across(rows[k + k // 2], vs).realizations.to_float32()

if mode == "devices_two":
    fm.init_devices([0, 0])
    fm.set_fusion(True)
    for k, a in arrays.items():
        vs = [fm.DeviceVector.from_host(x) for x in a]
        everything("stored", k, vs)
        everything("pending", k, [v.v1s1("MULT_S", 2.0) for v in vs])
elif mode == "threads":
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    owned = {k: [fm.DeviceVector.from_host(x) for x in a] for k, a in arrays.items()}
    pend = {k: [v.v1s1("MULT_S", 2.0) for v in vs] for k, vs in owned.items()}      # pending, owned by the main thread's engine
    def other():
        for k in arrays:
            everything("stored", k, owned[k])
            everything("pending", k, pend[k])
    t = threading.Thread(target=other); t.start(); t.join()
np.savez(out_path, **res)
print("RESULT " + json.dumps({"keys": len(res)}))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  Behind fmhip_init_devices({0, 0}) both passes run per shard and the results are the definition's; with thread
    engines a thread that owns neither the vectors nor the pending ones orders and selects, and the outputs are read on the main thread."""
    from test_cross_order_cpu import cross_data as data
    script = tmp_path / "fronts.py"
    script.write_text(_FRONTS % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    out_path = tmp_path / (mode + ".npz")
    r = subprocess.run([sys.executable, str(script), mode, str(out_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = dict(np.load(out_path))
    for k in (3, 17):
        a = data(k, 4099, np.random.default_rng(900 + k))
        for tag, arrays in (("stored", a), ("pending", [(x * np.float32(2.0)).astype(np.float32) for x in a])):
            want = gpu.cross_order_statistics_host(arrays, range(k), True, True)
            for j, w in enumerate(want): assert (bits(res[f"{tag}_{k}_{j}"]) == bits(w)).all(), (mode, tag, k, j)
            assert (bits(res[f"{tag}_{k}_select"]) == bits(gpu.cross_select_host(want[k + k // 2], arrays))).all(), (mode, tag, k)


# ---------------------------------------------------------------- the driver
DATES = [k / 3 for k in range(1, 10)]
PATHS, SEED = 1 << 18, 3141
# montecarlo.bermudan_max_call_mc(bm, [100, 100], 0.05, 0.10, 0.20, DATES, 100, basis_order=3) of the commit before ordered_states existed, fusion
# on, on these paths: (value, standard error), recorded from that commit's code on an MI355X
PARENT_DEFAULT = (float.fromhex("0x1.b57f149da26d7p+3"), float.fromhex("0x1.db93eb94d3b7ap-6"))
# benchmarks/cross_order_restatement.py (float64 numpy, 8 seeds, this configuration; profiles/cross_order.json "restatement"): the gaps
# ordered − unordered are 0.0821 … 0.1094, standard errors up to 0.0296 — half the smallest gap is above one standard error
MARGIN = 0.5 * 0.08208194768418231


@pytest.fixture(scope="module")
def max_call(gpu):
    """The runs the driver tests share: 2 assets, 9 dates, degree 3, 2^18 paths, the same paths for every run; one asset at 2^14."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    prev = gpu.set_fusion(True)
    try:
        bm = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 9, 1.0 / 3), 2, PATHS, SEED)
        small = gpu.BrownianMotionHip(gpu.TimeDiscretization(0.0, 9, 1.0 / 3), 3, 1 << 14, SEED)
        run = lambda motion, s0, **kw: mc.bermudan_max_call_mc(motion, s0, 0.05, 0.10, 0.20, DATES, 100.0, basis_order=3, **kw)
        out = {"unordered": run(bm, [100.0, 100.0]), "ordered": run(bm, [100.0, 100.0], ordered_states=True),
               "one_pass": run(small, [100.0] * 3, ordered_states=True, one_pass_basis=True),
               "one_asset": run(small, [100.0]), "one_asset_ordered": run(small, [100.0], ordered_states=True),
               "european": mc.bermudan_max_call_mc(small, [100.0] * 3, 0.05, 0.10, 0.20, DATES[-1:], 100.0, ordered_states=True),
               "best_of": mc.best_of_call_mc(small, [100.0] * 3, 0.05, 0.10, 0.20, DATES[-1], 100.0)}
        with knob_off():
            out["ordered_off"] = run(bm, [100.0, 100.0], ordered_states=True)
            out["one_pass_off"] = run(small, [100.0] * 3, ordered_states=True, one_pass_basis=True)
            out["unordered_off"] = run(bm, [100.0, 100.0])
    finally:
        gpu.set_fusion(prev)
    for name, value in out.items(): print(name, value, [float(x).hex() for x in value[:2]])
    return out


def test_the_default_is_the_value_of_the_commit_before(max_call):
    assert max_call["unordered"] == PARENT_DEFAULT
    assert max_call["unordered_off"] == PARENT_DEFAULT                    # the default route does not read the knob


def test_ordered_states_equal_their_knob_off_run_bit_for_bit(max_call):
    assert max_call["ordered"] == max_call["ordered_off"]
    assert max_call["one_pass"] == max_call["one_pass_off"]


def test_with_one_asset_ordered_and_unordered_are_identical(max_call):
    assert max_call["one_asset"] == max_call["one_asset_ordered"]


def test_best_of_call_is_the_one_date_max_call(max_call):
    value, error, shares = max_call["best_of"]
    assert (value, error) == max_call["european"]
    assert abs(sum(shares) - 1.0) <= 1e-6 and all(abs(s - 1.0 / 3) < 0.02 for s in shares)          # three exchangeable assets, 2^14 paths


def test_ordered_states_raise_the_lower_bound_by_the_restatements_margin(max_call):
    """The pricing claim: on the same paths the basis of ordered prices gives a better exercise policy, so a higher lower bound.  README:
    13.748 ± 0.029 against a literature value of about 13.90 (from memory; not asserted)."""
    (unordered, se_u), (ordered, se_o) = max_call["unordered"], max_call["ordered"]
    print(f"max-call, 2 assets, 9 dates, degree 3, {PATHS} paths: unordered {unordered:.4f} ± {se_u:.4f}, ordered {ordered:.4f} ± {se_o:.4f}, gap {ordered - unordered:.4f}, margin {MARGIN:.4f}")
    assert ordered - unordered > MARGIN
