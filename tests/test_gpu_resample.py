"""The device resampling on the GPU (include/fmhip.h: fmhip_resample; csrc/resample_kernel.hip): the device's ancestors and
gathered vectors EQUAL fmhip_resample_host's, the definition, bit for bit — over a grid of sizes around every boundary of the tree, every
scheme and equal weights, 0, 1 and 8 companions and every weight family; targets constructed to equal a chunk's last prefix; degenerate
totals; the inputs and the prefix calls unchanged; every refusal made on the host (nothing launched); the mirror's FMHIP_DEVICE_RESAMPLE=0
and =1 to the last bit, the filter drivers among them; the bootstrap filter against the Kalman filter; thread engines and device lists."""
import ctypes as C
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from test_resample_cpu import (A, CHUNK, P0, PARTICLES, Q, QUIET_NAN, R, SEEDS, STEPS, THREE_CHUNKS, TWO_CHUNKS, bits, families, kalman_observations,
                               values_for)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYSTEMATIC, STRATIFIED, MULTINOMIAL = 0, 1, 2
SCHEMES = (SYSTEMATIC, STRATIFIED, MULTINOMIAL)


def device(gpu, w, scheme, m, offset, u, values, ancestors=True):
    """fmhip_resample through ctypes on uploaded (or given) vectors: (outs as uint32 bits, ancestors as uint32 bits or None, total)."""
    up = lambda a: a if (a is None or isinstance(a, gpu.DeviceVector)) else gpu.DeviceVector.from_host(np.ascontiguousarray(a, dtype=np.float32))
    W, U, V = up(w), up(u if scheme != SYSTEMATIC else None), [up(v) for v in values]
    hv = (C.c_int64 * max(len(V), 1))(*[v.handle for v in V])
    out = (C.c_int64 * max(len(V), 1))()
    anc, total = C.c_int64(0), C.c_double(-1.0)
    gpu._native.check(gpu.lib().fmhip_resample(W.handle if W else 0, scheme, m, offset, U.handle if U else 0, hv if V else None, len(V), out if V else None,
                                               C.byref(anc) if ancestors else None, C.byref(total)))
    outs = [bits(gpu.DeviceVector(int(out[i]), m).to_float32()) for i in range(len(V))]
    return outs, (bits(gpu.DeviceVector(anc.value, m).to_float32()) if ancestors else None), total.value


def ancestors_as_bits(a):
    f = a.astype(np.float32)
    return np.where(a >= 0, f.view(np.uint32), np.uint32(QUIET_NAN)).astype(np.uint32)


def check(gpu, w, scheme, m, offset, u, values, what, ancestors=True):
    n = w.size if w is not None else values[0].size
    ancestors = ancestors and n <= (1 << 24)
    want_outs, want_a, want_total = gpu.resample_host(w, values, m, scheme, offset, u if scheme != SYSTEMATIC else None)
    outs, a, total = device(gpu, w, scheme, m, offset, u, values, ancestors or not values)
    assert np.float64(total).view(np.uint64) == np.float64(want_total).view(np.uint64), what
    if a is not None: assert (a == ancestors_as_bits(want_a)).all(), (what, np.flatnonzero(a != ancestors_as_bits(want_a))[:5])
    assert len(outs) == len(want_outs)
    for k, (o, wo) in enumerate(zip(outs, want_outs)):
        assert (o == bits(wo)).all(), (what, k, np.flatnonzero(o != bits(wo))[:5])


def uniforms(m, rng):
    u = rng.random(m, dtype=np.float32)
    if m > 4: u[[0, 1, 2, 3]] = [np.nan, -0.5, 1.0, np.nextafter(np.float32(1), np.float32(0))]
    return u


# the n × m grid of the CPU test, thinned: every n, with m below, at and above it, at the tile of the gather (1024) and beside it
GRID = [(1, 1), (1, 65), (7, 63), (8, 64), (9, 36), (511, 1), (511, 2044), (512, 512), (513, 128), (513, 65), (2047, 2047), (2048, 8192), (2048, 1023),
        (2049, 1024), (2049, 1025), (3 * 2048 + 5, 64), (3 * 2048 + 5, 3 * 2048 + 5), (TWO_CHUNKS - 1, 4096), (TWO_CHUNKS, 63), (TWO_CHUNKS, TWO_CHUNKS), (TWO_CHUNKS, 4 * TWO_CHUNKS),
        (THREE_CHUNKS, 1), (THREE_CHUNKS, THREE_CHUNKS), (THREE_CHUNKS, THREE_CHUNKS // 4), (THREE_CHUNKS, 4 * THREE_CHUNKS), (100_003, 65), (100_003, 100_003),
        (300_007, 2049), (65, 300_007), (1 << 20, 1 << 18)]


@pytest.mark.parametrize("n,m", GRID)
def test_device_equals_the_host_definition(gpu, n, m):
    rng = np.random.default_rng(1000 * n + m)
    fams = list(families(n, rng))
    values = values_for(n, rng, 8)
    u = uniforms(m, rng)
    case = (n + m) % len(fams)
    for scheme in SCHEMES:
        for n_values in (0, 1, 8):
            name, w = fams[case % len(fams)]; case += 1
            offset = [0.0, 0.5, float(np.nextafter(1.0, 0.0)), float(rng.random())][case % 4]
            check(gpu, w, scheme, m, offset, u, values[:n_values], (name, scheme, n_values))
    for k, scheme in enumerate(SCHEMES):
        check(gpu, None, scheme, m, 0.25, u, values[:(1, 8, 2)[k]], ("equal weights", scheme), ancestors=k != 1)


def test_every_family_and_scheme_at_three_chunks(gpu):
    n = THREE_CHUNKS + 77
    rng = np.random.default_rng(5)
    values = values_for(n, rng, 2)
    for name, w in families(n, rng):
        for scheme in SCHEMES:
            check(gpu, w, scheme, n + 5, 0.375, uniforms(n + 5, rng), values, (name, scheme))


def test_a_large_odd_size(gpu):
    n = m = (1 << 20) + 3
    rng = np.random.default_rng(20)
    fams = dict(families(n, rng))
    values = values_for(n, rng, 2)
    u = uniforms(m, rng)
    check(gpu, fams["concentrated"], SYSTEMATIC, m, 0.7, u, values, "systematic")
    check(gpu, fams["wide range"], STRATIFIED, m, 0.0, u, values[:1], "stratified")
    check(gpu, fams["half zeros"], MULTINOMIAL, m, 0.0, u, values[:1], "multinomial")
    check(gpu, None, MULTINOMIAL, m, 0.0, u, values[:1], "bootstrap")


def test_chunks_of_more_than_two_tiles(gpu):
    """Above 2^22 elements a chunk is longer than two tiles: the bisection inside a chunk runs more steps (the one size here above 2^20)."""
    n, m = (1 << 22) + (1 << 21) + 5, 1 << 16
    rng = np.random.default_rng(21)
    w = rng.random(n, dtype=np.float32); w[rng.random(n) < 0.3] = 0.0
    x = rng.standard_normal(n).astype(np.float32)
    u = uniforms(m, rng)
    for scheme in SCHEMES:
        check(gpu, w, scheme, m, 0.125, u, [x], scheme)


def test_targets_that_equal_a_chunks_last_prefix(gpu):
    """Equal dyadic weights, offset 0, m = n a power of two: every t_j equals P[j-1] exactly — the last prefix of a chunk for j = 4096, 8192,
    12288 — and the strict > picks path j, the first of the NEXT chunk."""
    n = 4 * CHUNK
    w = np.full(n, 0.25, dtype=np.float32)
    x = np.arange(n, dtype=np.float32)
    (out,), a, total = device(gpu, w, SYSTEMATIC, n, 0.0, None, [x])
    assert total == 0.25 * n and (out == bits(x)).all() and (a == bits(x)).all()
    (out,), a, _ = device(gpu, w, SYSTEMATIC, 2 * n, 0.0, None, [x])
    assert (out == bits((np.arange(2 * n) // 2).astype(np.float32))).all()
    P = np.cumsum(w.astype(np.float64))
    u = np.concatenate([(P[[CHUNK - 1, 2 * CHUNK - 1, 3 * CHUNK - 1, 0, n - 2]] / P[-1]), [0.0]]).astype(np.float32)      # exact: dyadic
    (out,), a, _ = device(gpu, w, MULTINOMIAL, u.size, 0.0, u, [x])
    assert out.view(np.float32).tolist() == [CHUNK, 2 * CHUNK, 3 * CHUNK, 1, n - 1, 0]
    check(gpu, w, MULTINOMIAL, u.size, 0.0, u, [x], "at the chunks' last prefixes")


def test_degenerate_totals(gpu):
    n, m = THREE_CHUNKS, 5000
    rng = np.random.default_rng(1)
    x = rng.standard_normal(n).astype(np.float32)
    u = uniforms(m, rng)
    inf = np.ones(n, dtype=np.float32); inf[CHUNK + 5] = np.inf
    for w, is_total in ((np.zeros(n, dtype=np.float32), lambda t: t == 0.0), (np.full(n, -1.0, dtype=np.float32), lambda t: t == 0.0),
                        (np.full(n, np.nan, dtype=np.float32), lambda t: t == 0.0), (inf, lambda t: t == math.inf)):
        for scheme in SCHEMES:
            (out,), a, total = device(gpu, w, scheme, m, 0.5, u, [x])                  # (the status is FMHIP_OK)
            assert is_total(total) and (out == QUIET_NAN).all() and (a == QUIET_NAN).all()
            check(gpu, w, scheme, m, 0.5, u, [x], "degenerate")


def test_inputs_and_prefix_calls_are_unchanged(gpu):
    n = THREE_CHUNKS + 9
    rng = np.random.default_rng(2)
    w = dict(families(n, rng))["NaN, negative, -0.0"]
    x = values_for(n, rng, 1)[0]
    u = uniforms(n, rng)
    W, X, U = (gpu.DeviceVector.from_host(a) for a in (w, x, u))
    before, total_before = gpu.cumulative_sums(W, with_total=True)
    before = bits(before.to_float32())
    for scheme in SCHEMES:
        device(gpu, W, scheme, n, 0.5, U, [X])
    after, total_after = gpu.cumulative_sums(W, with_total=True)
    assert (bits(after.to_float32()) == before).all() and (np.isnan(total_before) and np.isnan(total_after) or total_before == total_after)
    assert (bits(W.to_float32()) == bits(w)).all() and (bits(X.to_float32()) == bits(x)).all() and (bits(U.to_float32()) == bits(u)).all()


def test_pending_operands_give_the_bits_of_materialised_ones(gpu):
    prev = gpu.set_fusion(True)
    try:
        n = TWO_CHUNKS + 3
        rng = np.random.default_rng(3)
        w, x = rng.random(n, dtype=np.float32), rng.standard_normal(n).astype(np.float32)
        W, X = gpu.DeviceVector.from_host(w).v1s1("MULT_S", 2.0), gpu.DeviceVector.from_host(x).v1s1("ADD_S", 1.0)
        outs, a, total = device(gpu, W, SYSTEMATIC, n, 0.25, None, [X])
        want_outs, want_a, want_total = gpu.resample_host(W.to_float32(), [X.to_float32()], n, SYSTEMATIC, 0.25)
        assert (outs[0] == bits(want_outs[0])).all() and (a == ancestors_as_bits(want_a)).all() and total == want_total
    finally:
        gpu.set_fusion(prev)


def test_refusals_are_made_on_the_host(gpu):
    N = gpu._native
    lib = gpu.lib()
    n = m = 1000
    w, x, u = (gpu.DeviceVector.from_host(np.random.default_rng(k).random(n, dtype=np.float32)) for k in range(3))
    longer = gpu.DeviceVector.from_host(np.ones(n + 1, dtype=np.float32))
    before = gpu.pool_stats()
    out, anc, total = (C.c_int64 * 9)(), C.c_int64(0), C.c_double(-1.0)
    one, nine, with_zero = (C.c_int64 * 1)(x.handle), (C.c_int64 * 9)(*[x.handle] * 9), (C.c_int64 * 2)(x.handle, 0)
    call = lambda weights, scheme, m_, offset, uni, values, n_values, outs, a=C.byref(anc): lib.fmhip_resample(weights, scheme, m_, offset, uni, values, n_values, outs, a, C.byref(total))
    bad = N.ERR_INVALID_ARGUMENT
    assert call(w.handle, 3, m, 0.5, u.handle, one, 1, out) == bad                      # an unknown scheme
    assert call(w.handle, -1, m, 0.5, u.handle, one, 1, out) == bad
    for size in (0, -1, 1 << 31):
        assert call(w.handle, 0, size, 0.5, 0, one, 1, out) == bad                      # m outside 1 … 2^31 - 1
    assert call(w.handle, 0, m, 0.5, 0, nine, 9, out) == bad                            # n_values outside 0 … 8
    assert call(w.handle, 0, m, 0.5, 0, one, -1, out) == bad
    assert call(w.handle, 0, m, 0.5, 0, None, 0, None, None) == bad                     # nothing asked for
    assert call(0, 2, m, 0.0, u.handle, None, 0, None) == bad                           # neither weights nor a value vector
    for offset in (1.0, -0.25, math.nan, math.inf):
        assert call(w.handle, 0, m, offset, 0, one, 1, out) == bad                      # an offset outside [0, 1) or not finite
        assert call(w.handle, 1, m, offset, u.handle, one, 1, out) == bad               # (whatever the scheme)
    for scheme in (1, 2):
        assert call(w.handle, scheme, m, 0.0, 0, one, 1, out) == bad                    # uniforms == 0 with a scheme that needs them
    assert call(w.handle, 0, m, 0.5, 0, None, 1, out) == bad                            # NULL pointers
    assert call(w.handle, 0, m, 0.5, 0, one, 1, None) == bad
    assert call(w.handle, 0, m, 0.5, 0, with_zero, 2, out) == bad
    assert call(w.handle, 0, m, 0.5, 0, (C.c_int64 * 1)(longer.handle), 1, out) == N.ERR_SIZE_MISMATCH       # a value vector whose size is not n
    assert call(w.handle, 2, m + 1, 0.0, u.handle, one, 1, out) == N.ERR_SIZE_MISMATCH                      # uniforms whose size is not m
    assert call(w.handle + 12345, 0, m, 0.5, 0, one, 1, out) == N.ERR_INVALID_HANDLE
    assert call(w.handle, 2, m, 0.0, u.handle + 12345, one, 1, out) == N.ERR_INVALID_HANDLE
    assert call(w.handle, 0, m, 0.5, 0, (C.c_int64 * 1)(x.handle + 12345), 1, out) == N.ERR_INVALID_HANDLE
    # ancestors beyond 2^24 elements (an uninitialised vector: nothing reads it)
    huge = C.c_int64(0)
    N.check(lib.fmhip_vec_create_uninitialized((1 << 24) + 1, C.byref(huge)))
    try:
        assert call(huge.value, 0, m, 0.5, 0, None, 0, None) == bad
    finally:
        N.check(lib.fmhip_vec_release(huge.value))
    with pytest.raises(ValueError): gpu.resample(w, [x], scheme="systematic")           # the mirror: no offset
    with pytest.raises(ValueError): gpu.resample(w, [x], scheme="stratified")
    with pytest.raises(ValueError): gpu.resample(w, [longer], offset=0.5)
    # a communicator of two ranks: a carry between the ranks is not built
    try:
        gpu.set_expectation_comm(2, 0, lambda local: np.stack([local, local]))
        assert call(w.handle, 0, m, 0.5, 0, one, 1, out) == N.ERR_UNSUPPORTED
        assert call(0, 2, m, 0.0, u.handle, one, 1, out) == N.ERR_UNSUPPORTED
    finally:
        gpu.set_expectation_comm(1, 0, None)
    after = gpu.pool_stats()
    assert after.n_kernel_launches == before.n_kernel_launches and after.n_live_vectors == before.n_live_vectors      # nothing was launched for any of it
    assert list(out) == [0] * 9 and anc.value == 0 and total.value == -1.0
    assert call(w.handle, 0, m, 0.5, 0, one, 1, out) == N.OK and out[0] != 0 and anc.value != 0 and total.value > 0
    assert gpu.pool_stats().n_kernel_launches == after.n_kernel_launches + 1                                            # ONE armed launch per call
    N.check(lib.fmhip_vec_release(out[0])); N.check(lib.fmhip_vec_release(anc.value))


def test_a_given_up_vector_is_the_error_a_read_is(gpu):
    prev = gpu.set_fusion(True)
    try:
        base = gpu.DeviceVector.from_host(np.arange(1, 4097, dtype=np.float32))
        ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 4)]
        gpu.give_up_values(ys)
        gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
        for y in ys:
            try:
                y.to_float32()
                read_error = None
            except gpu.FmhipError as e:
                read_error = e.code
            for call in (lambda: gpu.resample(y, [base], offset=0.5), lambda: gpu.resample(base, [y], offset=0.5)):
                if read_error is None:
                    call()
                else:
                    with pytest.raises(gpu.FmhipError) as info:
                        call()
                    assert info.value.code == read_error and "given up" in str(info.value)
    finally:
        gpu.set_fusion(prev)


def test_the_mirror(gpu, monkeypatch):
    monkeypatch.setenv("FMHIP_DEVICE_RESAMPLE", "1")
    n = 5000
    rng = np.random.default_rng(9)
    w, x, y = rng.random(n, dtype=np.float32), rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    W, X, Y = gpu.RandomVariableHip(1.0, w), gpu.RandomVariableHip(2.0, x), gpu.DeviceVector.from_host(y)
    u = rng.random(700, dtype=np.float32)
    U = gpu.DeviceVector.from_host(u)
    (ox, oy), anc, total = gpu.systematic_resample(W, [X, Y], 0.3, ancestors=True)
    want, a, t = gpu.resample_host(w, [x, y], n, "systematic", 0.3)
    assert ox.getFiltrationTime() == 2.0 and oy.getFiltrationTime() == 1.0 and anc.getFiltrationTime() == 1.0 and ox.size() == n
    assert (bits(ox.realizations.to_float32()) == bits(want[0])).all() and (bits(oy.realizations.to_float32()) == bits(want[1])).all()
    assert (anc.realizations.to_float32() == a).all() and total == t
    (ox,), total = gpu.stratified_resample(W, [X], U)
    assert ox.size() == 700 and (bits(ox.realizations.to_float32()) == bits(gpu.resample_host(w, [x], 700, "stratified", None, u)[0][0])).all()
    (ox,), total = gpu.multinomial_resample(W, [X], U)
    assert (bits(ox.realizations.to_float32()) == bits(gpu.resample_host(w, [x], 700, "multinomial", None, u)[0][0])).all()
    ox, oy = gpu.bootstrap_resample([X, Y], U)
    pick = np.minimum(np.floor(u.astype(np.float64) * n).astype(np.int64), n - 1)
    assert (bits(ox.realizations.to_float32()) == bits(x[pick])).all() and (bits(oy.realizations.to_float32()) == bits(y[pick])).all()
    w64 = w.astype(np.float64)
    assert gpu.effective_sample_size(W) == pytest.approx(w64.sum() ** 2 / (w64 ** 2).sum(), rel=1e-12)
    assert gpu.effective_sample_size(gpu.DeviceVector.filled(n, 0.5)) == n


# ---------------------------------------------------------------- the knob, in a process of its own per setting
_KNOB = r'''
import importlib, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
out_path = sys.argv[1]
fm.init(0)
before = fm.pool_stats().n_kernel_launches
rng = np.random.default_rng(31)
n, m = 12_345, 7_001
w = rng.random(n, dtype=np.float32); w[rng.random(n) < 0.3] = 0.0; w[5] = np.nan; w[6] = -1.0
x, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
u = rng.random(m, dtype=np.float32); u[0] = np.nan; u[1] = 1.0; u[2] = -1.0
W, X, Y, U = (fm.DeviceVector.from_host(a) for a in (w, x, y, u))
res = {}
for scheme in ("systematic", "stratified", "multinomial"):
    (ox, oy), anc, total = fm.resample(W, [X, Y], m=m, scheme=scheme, offset=0.625 if scheme == "systematic" else None, uniforms=None if scheme == "systematic" else U, ancestors=True)
    res[scheme + "_x"], res[scheme + "_y"], res[scheme + "_a"], res[scheme + "_t"] = ox.realizations.to_float32(), oy.realizations.to_float32(), anc.realizations.to_float32(), np.array([total])
(ox,), total = fm.resample(fm.DeviceVector.from_host(np.zeros(n, dtype=np.float32)), [X], offset=0.5)
res["degenerate_x"], res["degenerate_t"] = ox.realizations.to_float32(), np.array([total])
bx, by = fm.bootstrap_resample([X, Y], U)
res["bootstrap_x"], res["bootstrap_y"] = bx.realizations.to_float32(), by.realizations.to_float32()
particles, steps = 1 << 12, 20
obs = np.random.default_rng(4).standard_normal(steps) * 0.8
bm = fm.BrownianMotionHip(fm.TimeDiscretization(0.0, steps + 1, 1.0), 1, particles, 3141)
res["filter"] = np.array([mc.particle_filter_log_likelihood(obs, 0.9, 0.25, 0.25, 1.0, bm, 7, scheme) for scheme in ("systematic", "stratified", "multinomial")])
returns = np.random.default_rng(5).standard_normal(steps) * 0.01
res["sv"] = np.array([mc.stochastic_volatility_log_likelihood(returns, -9.0, 0.95, 0.2, bm, 8, scheme) for scheme in ("systematic", "multinomial")])
np.savez(out_path, **res)
print("RESULT " + json.dumps({"knob": fm.device_resample(), "launches": fm.pool_stats().n_kernel_launches - before}))
fm.shutdown()
'''


def _run(tmp_path, text, name, args=(), env=None):
    script = tmp_path / (name + ".py")
    script.write_text(text % {"root": ROOT})
    out_path = tmp_path / (name + "_" + "_".join(args) + ".npz")
    r = subprocess.run([sys.executable, str(script), *args, str(out_path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    return info, dict(np.load(out_path))


def test_the_knob_gives_the_same_bits(gpu, tmp_path):
    """resample in every scheme, a degenerate total, bootstrap_resample and both filter drivers (2^12 particles × 20 steps, every scheme) in a
    fresh process per setting of FMHIP_DEVICE_RESAMPLE — the knob is in the environment at the process's start — : the same bits, the
    log-likelihoods to the last one."""
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    on_info, on = _run(tmp_path / "on", _KNOB, "knob", env={"FMHIP_DEVICE_RESAMPLE": "1"})
    off_info, off = _run(tmp_path / "off", _KNOB, "knob", env={"FMHIP_DEVICE_RESAMPLE": "0"})
    assert on_info["knob"] is True and off_info["knob"] is False and on_info["launches"] > off_info["launches"]
    assert sorted(on) == sorted(off) and len(on) == 18
    for key in on:
        a, b = on[key], off[key]
        same = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a.view(np.uint64) == b.view(np.uint64))
        assert a.shape == b.shape and same.all(), key
    assert np.isfinite(on["filter"]).all() and np.isfinite(on["sv"]).all()
    assert (bits(on["degenerate_x"]) == QUIET_NAN).all() and on["degenerate_t"][0] == 0.0


def test_the_particle_filter_against_the_kalman_filter(gpu, monkeypatch):
    """16 seeds × 4096 particles × 50 steps: the device log-likelihoods equal the host-path ones bit for bit, and the mean of
    exp(loglik − kalman) lies within 4 of its own standard errors of 1."""
    mc = importlib.import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    ys = kalman_observations()
    exact = mc.kalman_log_likelihood(ys, A, Q, R, P0)
    td = gpu.TimeDiscretization(0.0, STEPS + 1, 1.0)
    def run(seed):
        return mc.particle_filter_log_likelihood(ys, A, Q, R, P0, gpu.BrownianMotionHip(td, 1, PARTICLES, 100 + seed), 1000 + seed)
    monkeypatch.setenv("FMHIP_DEVICE_RESAMPLE", "1")
    launches = gpu.pool_stats().n_kernel_launches
    on = np.array([run(seed) for seed in range(SEEDS)])
    on_launches = gpu.pool_stats().n_kernel_launches - launches
    monkeypatch.setenv("FMHIP_DEVICE_RESAMPLE", "0")
    launches = gpu.pool_stats().n_kernel_launches
    off = np.array([run(seed) for seed in range(SEEDS)])
    assert on_launches > gpu.pool_stats().n_kernel_launches - launches                       # the resample launches, on the device path only
    assert (on.view(np.uint64) == off.view(np.uint64)).all()
    ratios = np.exp(on - exact)
    mean, error = ratios.mean(), ratios.std(ddof=1) / math.sqrt(SEEDS)
    print(f"exp(loglik - kalman): {mean:.4f} +- {error:.4f}")
    assert abs(mean - 1.0) <= 4.0 * error, (mean, error)


# ---------------------------------------------------------------- the fronts: a device list, thread engines
_FRONTS = r'''
import ctypes as C, importlib, json, os, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode, out_path = sys.argv[1], sys.argv[2]
N = fm._native
n, m = 100_003, 50_001
rng = np.random.default_rng(77)
w = rng.random(n, dtype=np.float32); w[rng.random(n) < 0.4] = 0.0
x = rng.standard_normal(n).astype(np.float32)
u = rng.random(m, dtype=np.float32)
res, info = {}, {}

def everything(tag, W, X, U):
    for scheme in ("systematic", "stratified", "multinomial"):
        (ox,), anc, total = fm.resample(W, [X], m=m, scheme=scheme, offset=0.5 if scheme == "systematic" else None, uniforms=None if scheme == "systematic" else U, ancestors=True)
        res[tag + scheme + "_x"], res[tag + scheme + "_a"], res[tag + scheme + "_t"] = ox.realizations.to_float32(), anc.realizations.to_float32(), np.array([total])
    res[tag + "bootstrap_x"] = fm.bootstrap_resample([X], U)[0].realizations.to_float32()

if mode == "devices_one":
    fm.init_devices([0])
    fm.set_fusion(True)
    W, X, U = (fm.DeviceVector.from_host(a) for a in (w, x, u))
    everything("stored_", W, X, U)
    everything("pending_", W.v1s1("MULT_S", 2.0), X.v1s1("MULT_S", 2.0), U)
elif mode == "devices_two":
    fm.init_devices([0, 0])
    lib = fm.lib()
    W, X, U = (fm.DeviceVector.from_host(a) for a in (w, x, u))
    W.to_float32(); X.to_float32(); U.to_float32()
    before = fm.pool_stats()
    out, anc, total = C.c_int64(0), C.c_int64(0), C.c_double(-1.0)
    hv = (C.c_int64 * 1)(X.handle)
    info["status"] = [lib.fmhip_resample(W.handle, 0, m, 0.5, 0, hv, 1, C.byref(out), C.byref(anc), C.byref(total)),
                      lib.fmhip_resample(W.handle, 1, m, 0.0, U.handle, None, 0, None, C.byref(anc), None),
                      lib.fmhip_resample(0, 2, m, 0.0, U.handle, hv, 1, C.byref(out), None, C.byref(total))]
    info["unsupported"] = N.ERR_UNSUPPORTED
    info["message"] = lib.fmhip_last_error().decode("utf-8", "replace")
    after = fm.pool_stats()
    info["launches"] = [before.n_kernel_launches, after.n_kernel_launches]
    info["live"] = [before.n_live_vectors, after.n_live_vectors]
    info["outputs"] = [out.value, anc.value, total.value]
    os.environ["FMHIP_DEVICE_RESAMPLE"] = "0"                # the documented fallback: through reads and uploads, on any device list
    everything("stored_", W, X, U)
elif mode == "threads":
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    W, X, U = (fm.DeviceVector.from_host(a) for a in (w, x, u))
    PW, PX = W.v1s1("MULT_S", 2.0), X.v1s1("MULT_S", 2.0)     # pending, owned by the main thread's engine
    kept = {}
    def other():
        for tag, (a, b) in (("stored_", (W, X)), ("pending_", (PW, PX))):
            for scheme in ("systematic", "stratified", "multinomial"):
                kept[tag + scheme] = fm.resample(a, [b], m=m, scheme=scheme, offset=0.5 if scheme == "systematic" else None, uniforms=None if scheme == "systematic" else U, ancestors=True)
            kept[tag + "bootstrap"] = fm.bootstrap_resample([b], U)
    t = threading.Thread(target=other); t.start(); t.join()
    for tag in ("stored_", "pending_"):                       # read back on the main thread
        for scheme in ("systematic", "stratified", "multinomial"):
            (ox,), anc, total = kept[tag + scheme]
            res[tag + scheme + "_x"], res[tag + scheme + "_a"], res[tag + scheme + "_t"] = ox.realizations.to_float32(), anc.realizations.to_float32(), np.array([total])
        res[tag + "bootstrap_x"] = kept[tag + "bootstrap"][0].realizations.to_float32()
    kept.clear()
np.savez(out_path, **res)
print("RESULT " + json.dumps(info))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices_one", "devices_two", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """In a process of its own.  A device list of ONE shard is that shard's call: everything equals the definition, on stored and on pending
    operands.  A list {0, 0} answers FMHIP_ERR_UNSUPPORTED — nothing launched, nothing left behind — and the mirror's host path
    (FMHIP_DEVICE_RESAMPLE=0) gives the definition's results there.  Thread engines: a thread that owns none of the vectors resamples them —
    routed and equal; the outputs are read on the main thread."""
    n, m = 100_003, 50_001
    rng = np.random.default_rng(77)
    w = rng.random(n, dtype=np.float32); w[rng.random(n) < 0.4] = 0.0
    x = rng.standard_normal(n).astype(np.float32)
    u = rng.random(m, dtype=np.float32)
    info, res = _run(tmp_path, _FRONTS, "fronts", args=(mode,))
    tags = {"devices_one": ("stored_", "pending_"), "devices_two": ("stored_",), "threads": ("stored_", "pending_")}[mode]
    for tag in tags:
        ww, xx = (w, x) if tag == "stored_" else ((w * np.float32(2.0)).astype(np.float32), (x * np.float32(2.0)).astype(np.float32))
        for scheme in ("systematic", "stratified", "multinomial"):
            (want,), a, total = gpu.resample_host(ww, [xx], m, scheme, 0.5 if scheme == "systematic" else None, None if scheme == "systematic" else u)
            assert (bits(res[tag + scheme + "_x"]) == bits(want)).all(), (tag, scheme)
            assert (res[tag + scheme + "_a"] == a).all() and res[tag + scheme + "_t"][0] == total, (tag, scheme)
        assert (bits(res[tag + "bootstrap_x"]) == bits(gpu.resample_host(None, [xx], m, "multinomial", None, u)[0][0])).all(), tag
    if mode == "devices_two":
        assert info["status"] == [info["unsupported"]] * 3 and info["unsupported"] == gpu._native.ERR_UNSUPPORTED
        assert "shards" in info["message"]
        assert info["launches"][0] == info["launches"][1] and info["live"][0] == info["live"][1]
        assert info["outputs"] == [0, 0, -1.0]
