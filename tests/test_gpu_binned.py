"""Localized regression on the device (include/fmhip.h: fmhip_binned_cross_moments, fmhip_binned_evaluate): the device
against the host definition and the exact per-bin sums, bitwise determinism of a (bin, pair) sum, the piecewise evaluation against the
definition and against the recorded mult / addProduct chain, the estimator's device path against numpy's per-bin least squares and the
knob-off path, a device list, a two-rank communicator, and the Bermudan put against the tree.

Every test prints the figures it asserts on before it asserts (run with -s)."""
import json
import math
import os
import signal
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_binned_cpu import bin_of, edge_keys, evaluate_numpy, exact_and_bound, host_evaluate, host_moments, per_bin_lstsq

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 1023, 1025, 10**6 + 3, 2**24]


class limit:
    """A time limit of its own for one step on the device."""
    def __init__(self, seconds): self.seconds = seconds
    def __enter__(self):
        def over(*_): raise TimeoutError(f"a device step took more than {self.seconds} s")
        self.prev = signal.signal(signal.SIGALRM, over); signal.alarm(self.seconds)
    def __exit__(self, *a):
        signal.alarm(0); signal.signal(signal.SIGALRM, self.prev)


class knob_off:
    def __enter__(self):
        self.prev = os.environ.get("FMHIP_DEVICE_BINNED_MOMENTS")
        os.environ["FMHIP_DEVICE_BINNED_MOMENTS"] = "0"
    def __exit__(self, *a):
        if self.prev is None: del os.environ["FMHIP_DEVICE_BINNED_MOMENTS"]
        else: os.environ["FMHIP_DEVICE_BINNED_MOMENTS"] = self.prev


def bits(a): return np.asarray(a, dtype=np.float64).view(np.uint64)


def packed(S, T):
    iu = np.triu_indices(S.shape[1])
    return np.concatenate([S[:, iu[0], iu[1]], T.reshape(T.shape[0], -1)], axis=1)


def case(n, n_bins, seed):
    key, rng = edge_keys(n, seed)
    bounds = np.sort(rng.standard_normal(n_bins - 1))
    if n_bins >= 2: bounds[0] = 0.0
    if n_bins >= 16: bounds[3] = bounds[4]
    if n_bins == 64: bounds[1], bounds[-1] = -np.inf, np.inf
    bounds = np.sort(bounds)
    if n > 8 and n_bins > 1 and np.isfinite(bounds[n_bins // 2 - 1]): key[8 % n] = np.float32(bounds[n_bins // 2 - 1])
    return key, bounds, rng


def against_the_definition(gpu, n, n_bins):
    """Counts equal to the definition's and to fmhip_count_not_above's; sums within TWICE the bound of the definition's: the device and the
    definition are two summation orders of the same exact terms, each within m·2⁻⁵³·Σ|terms| of the exact sum.  Σ|terms| is taken by numpy in
    fp64 (relative error far below the factor 1 + 1e-6 it is given)."""
    key, bounds, rng = case(n, n_bins, n_bins + 3)
    x, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    with limit(240):
        K, X, Y = (gpu.DeviceVector.from_host(a) for a in (key, x, y))
        counts, S, T = gpu.binned_cross_moments(K, bounds, [None, X], [Y])
        not_above = K.count_not_above(np.concatenate([bounds, [np.inf]]))
    st, want_counts, want = host_moments(gpu, key, bounds, [None, x], [y])
    assert st == 0 and (counts == want_counts).all() and (counts == np.diff(np.concatenate([[0], not_above]))).all(), (n, n_bins)
    bins = bin_of_fast(key, bounds)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    ok = bins >= 0
    terms = [np.ones(n), xd, xd * xd, yd, xd * yd]
    tol = np.stack([np.bincount(bins[ok], weights=np.abs(t[ok]), minlength=n_bins) for t in terms], axis=1) * counts[:, None] * 2.0 ** -53 * (1 + 1e-6)
    err = np.abs(packed(S, T) - want)
    print(f"n={n} bins={n_bins}: max |device - definition| / (2 x bound) = {np.max(err / np.maximum(2 * tol, 1e-300)):.3g}")
    assert (err <= 2 * tol).all(), (n, n_bins)


def bin_of_fast(key, bounds):
    k = key.astype(np.float64)
    return np.where(np.isnan(k), -1, np.searchsorted(np.asarray(bounds, dtype=np.float64), k, side="left"))


@pytest.mark.parametrize("n", [1025, 10**6 + 3])
def test_all_keys_equal(gpu, n):
    """Every lane of every wave in ONE bin, every other bin empty — the key strictly inside a bin, and equal to a bound (it belongs below it)."""
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    key = np.full(n, 2.5, dtype=np.float32)
    sixteen = np.sort(np.concatenate([[2.5], np.linspace(-3.0, 6.0, 14)]))
    sixty_four = np.sort(np.concatenate([[2.5], np.linspace(-3.0, 6.0, 62)]))
    with limit(240):
        K, X, Y = (gpu.DeviceVector.from_host(a) for a in (key, x, y))
        for bounds, home in (([1.0, 2.5, 3.0], 1), ([1.0, 2.0, 3.0], 2), (sixteen, int(np.searchsorted(sixteen, 2.5))), (sixty_four, int(np.searchsorted(sixty_four, 2.5))), ([], 0)):
            counts, S, T = gpu.binned_cross_moments(K, bounds, [None, X, Y], [Y, X])
            want_counts, want, tol = exact_and_bound(key, bounds, [None, x, y], [y, x])
            assert counts[home] == n and counts.sum() == n and (counts == want_counts).all(), (n, len(bounds))
            got = packed(S, T)
            assert (np.abs(got - want) <= tol).all(), (n, len(bounds))
            assert (np.delete(got, home, axis=0) == 0.0).all()
            est = gpu.binned_evaluate(K, bounds, [None, X], np.arange(2 * (len(bounds) + 1), dtype=np.float64).reshape(-1, 2))
            st, ref = host_evaluate(gpu, key, bounds, [None, x], np.arange(2 * (len(bounds) + 1), dtype=np.float64).reshape(-1, 2))
            assert st == 0 and (est.to_float32().view(np.uint32) == ref.view(np.uint32)).all()


@pytest.mark.parametrize("n", SIZES)
def test_device_against_definition_and_exact_sums(gpu, n):
    for n_bins in (1, 2, 16, 64):
        if n == 2**24 and n_bins != 16:
            against_the_definition(gpu, n, n_bins)                    # math.fsum over 2²⁴ paths costs the host seconds per pair: one bin count takes it
            continue
        key, bounds, rng = case(n, n_bins, n_bins + n % 1000)
        shape = (2, 1) if n >= 10**6 else [(1, 0), (2, 1), (3, 1), (3, 4)][(n + n_bins) % 4]
        cols = [rng.standard_normal(n).astype(np.float32) for _ in range((shape[0] - 1 if shape[0] > 1 else 1) + shape[1])]
        xs_host = ([None] + cols[:shape[0] - 1]) if shape[0] > 1 else [cols[0]]
        ys_host = cols[len(cols) - shape[1]:] if shape[1] else []
        with limit(240):
            K = gpu.DeviceVector.from_host(key)
            dev = {id(c): gpu.DeviceVector.from_host(c) for c in cols}
            xs = [None if c is None else dev[id(c)] for c in xs_host]
            ys = [dev[id(c)] for c in ys_host]
            before = gpu.pool_stats().n_kernel_launches
            counts, S, T = gpu.binned_cross_moments(K, bounds, xs, ys)
            assert gpu.pool_stats().n_kernel_launches - before == 1
            not_above = K.count_not_above(np.concatenate([bounds, [np.inf]])) if n_bins > 1 else K.count_not_above([np.inf])
        st, want_counts, _ = host_moments(gpu, key, bounds, xs_host, ys_host)
        assert st == 0 and (counts == want_counts).all(), (n, n_bins)
        assert (counts == np.diff(np.concatenate([[0], not_above]))).all(), (n, n_bins)
        exact_counts, want, tol = exact_and_bound(key, bounds, xs_host, ys_host)
        got = packed(S, T)
        assert (counts == exact_counts).all()
        err = np.abs(got - want)
        print(f"n={n} bins={n_bins} shape={shape}: max error / bound = {np.max(err / np.maximum(tol, 1e-300)):.3g}")
        assert (err <= tol).all(), (n, n_bins, shape, np.max(err / np.maximum(tol, 1e-300)))


def test_pending_inputs_are_accepted_and_given_up_values_are_the_error(gpu):
    prev = gpu.set_fusion(True)
    try:
        with limit(120):
            n = 100_003
            key, bounds, rng = case(n, 16, 77)
            x = rng.standard_normal(n).astype(np.float32)
            K, X = gpu.DeviceVector.from_host(key), gpu.DeviceVector.from_host(x)
            want = gpu.binned_cross_moments(gpu.DeviceVector.from_host(key * np.float32(2.0)), bounds, [None, gpu.DeviceVector.from_host(x * np.float32(2.0))])
            got = gpu.binned_cross_moments(K.v1s1("MULT_S", 2.0), bounds, [None, X.v1s1("MULT_S", 2.0)])     # pending expressions: one flush, then the pass
            assert (got[0] == want[0]).all() and (bits(got[1]) == bits(want[1])).all()
            est = gpu.binned_evaluate(K.v1s1("MULT_S", 2.0), bounds, [None, X.v1s1("MULT_S", 2.0)], np.ones((16, 2)))
            st, ref = host_evaluate(gpu, key * np.float32(2.0), bounds, [None, x * np.float32(2.0)], np.ones((16, 2)))
            from conftest import assert_bits_equal
            assert_bits_equal(est.to_float32(), ref, "estimate of pending operands")
            base = gpu.DeviceVector.from_host(np.arange(4096, dtype=np.float32))
            ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 5)]
            gpu.give_up_values(ys)
            gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
            for k, y in enumerate(ys, start=1):
                try:
                    counts, S, _ = gpu.binned_cross_moments(base, [2047.0], [None, y])
                    assert counts.tolist() == [2048, 2048] and S[:, 0, 1].sum() == 4096 * 4095 / 2 + 4096 * k
                except gpu.FmhipError as e:
                    assert e.code == gpu._native.ERR_INVALID_ARGUMENT and "given up" in str(e)
            N = gpu._native
            with pytest.raises(gpu.FmhipError) as e: gpu.binned_cross_moments(K, [1.0, 0.0], [X])
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.binned_cross_moments(K, bounds, [X, gpu.DeviceVector.from_host(x[:-1])])
            assert e.value.code == N.ERR_SIZE_MISMATCH
            with pytest.raises(gpu.FmhipError) as e: gpu.binned_cross_moments(K, bounds, [X], [K.handle + (1 << 30)])
            assert e.value.code == N.ERR_INVALID_HANDLE
    finally:
        gpu.set_fusion(prev)


def test_a_bin_pair_sum_has_the_same_bits_whatever_else_the_call_names(gpu):
    with limit(240):
        n = 10**6 + 3
        rng = np.random.default_rng(12)
        key = rng.standard_normal(n).astype(np.float32)
        data = [rng.standard_normal(n).astype(np.float32) for _ in range(5)]
        K = gpu.DeviceVector.from_host(key)
        a, b, c, d, e = [gpu.DeviceVector.from_host(v) for v in data]
        b1, b2, b3 = -0.7, 0.1, 0.9
        _, S, _ = gpu.binned_cross_moments(K, [b1, b2, b3], [a, b])
        ref_ab, ref_aa = S[2, 0, 1], S[2, 0, 0]                       # the bin (b2, b3]
        # other vectors named; a and b as x, in other positions, among 18 products (sliced over blockIdx.y)
        _, S2, T2 = gpu.binned_cross_moments(K, [b1, b2, b3], [c, b, a], [d, e, c, b])
        assert bits(S2[2, 1, 2]) == bits(ref_ab) and bits(S2[2, 2, 2]) == bits(ref_aa) and bits(T2[2, 2, 3]) == bits(ref_ab)
        # swapped, and in the other role
        assert bits(gpu.binned_cross_moments(K, [b1, b2, b3], [b, a])[1][2, 0, 1]) == bits(ref_ab)
        assert bits(gpu.binned_cross_moments(K, [b1, b2, b3], [a], [b])[2][2, 0, 0]) == bits(ref_ab)
        assert bits(gpu.binned_cross_moments(K, [b1, b2, b3], [None, b], [a])[2][2, 1, 0]) == bits(ref_ab)
        # fewer and more other bins: the same bin (b2, b3]
        assert bits(gpu.binned_cross_moments(K, [b2, b3], [a, b])[1][1, 0, 1]) == bits(ref_ab)
        more = np.sort(np.concatenate([[b2, b3], np.linspace(-3, 0.0, 39), np.linspace(1.0, 3, 22)]))      # 63 bounds: 64 bins, sliced
        _, S64, _ = gpu.binned_cross_moments(K, more, [a, b])
        hit = [j for j in range(more.size) if j > 0 and more[j - 1] == b2 and more[j] == b3]
        assert hit and bits(S64[hit[0], 0, 1]) == bits(ref_ab) and bits(S64[hit[0], 0, 0]) == bits(ref_aa)
        # and from call to call
        assert bits(gpu.binned_cross_moments(K, [b1, b2, b3], [a, b])[1][2, 0, 1]) == bits(ref_ab)


@pytest.mark.parametrize("n", SIZES)
def test_evaluation_equals_the_definition_and_the_recorded_chain(gpu, n):
    from conftest import assert_bits_equal
    with limit(240):
        for n_bins, n_x in ((1, 3), (2, 1), (16, 2), (64, 3)):
            key, bounds, rng = case(n, n_bins, 5 * n_bins + n_x)
            cols = [(rng.standard_normal(n) * 3).astype(np.float32) for _ in range(n_x - (1 if n_x > 1 else 0))]
            xs_host = ([None] if n_x > 1 else []) + cols
            coefficients = rng.standard_normal((n_bins, n_x)) * 1.7
            K = gpu.DeviceVector.from_host(key)
            xs = [None if c is None else gpu.DeviceVector.from_host(c) for c in xs_host]
            before = gpu.pool_stats().n_kernel_launches
            out = gpu.binned_evaluate(K, bounds, xs, coefficients)
            assert gpu.pool_stats().n_kernel_launches - before == 1 and out.n == n
            st, want = host_evaluate(gpu, key, bounds, xs_host, coefficients)
            assert st == 0
            assert_bits_equal(out.to_float32(), want, f"n={n} bins={n_bins} n_x={n_x}")
            assert_bits_equal(want, evaluate_numpy(key, bounds, xs_host, coefficients), "definition")
        # one bin: the chain the existing estimator records for these coefficients, fused and eager
        f = gpu.RandomVariableHipFactory()
        for fusion in (False, True):
            prev = gpu.set_fusion(fusion)
            try:
                basis = [f.createRandomVariable(1.0)] + [f.createRandomVariable(0.0, c) for c in cols]
                beta = coefficients[0]
                ce = basis[0].mult(float(beta[0]))
                for i in range(1, len(basis)): ce = ce.addProduct(basis[i], float(beta[i]))
                nan_free = np.where(np.isnan(key), np.float32(0.0), key)
                got = gpu.binned_evaluate(gpu.DeviceVector.from_host(nan_free), [], [None] + [b.realizations for b in basis[1:]], beta)
                assert_bits_equal(got.to_float32(), ce.getRealizations().astype(np.float32), f"chain, fusion={fusion}")
            finally:
                gpu.set_fusion(prev)


def test_estimator_device_path_against_lstsq_and_the_knob_off_path(gpu):
    n = 200_000
    rng = np.random.default_rng(5)
    s = np.exp(0.3 * rng.standard_normal(n)).astype(np.float32)
    y = (np.maximum(1.05 - s, 0.0) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    f = gpu.RandomVariableHipFactory()
    for fusion in (False, True):
        prev = gpu.set_fusion(fusion)
        try:
            with limit(240):
                S, Y = f.createRandomVariable(0.0, s), f.createRandomVariable(0.0, y)
                for basis, cols in (([f.createRandomVariable(1.0), S], [np.ones(n, dtype=np.float32), s]),
                                    ([f.createRandomVariable(1.0), S, S.mult(S)], [np.ones(n, dtype=np.float32), s, s * s])):
                    est = gpu.MonteCarloConditionalExpectationLocalizedRegression(S, 16, basis)
                    counts = est.getBinCounts()
                    assert counts.sum() == n and (counts == np.bincount(bin_of(s, est.bounds), minlength=16)).all()
                    before = gpu.pool_stats().n_kernel_launches
                    beta = est.getLinearRegressionParameters(Y)
                    assert gpu.pool_stats().n_kernel_launches - before <= 2          # the pass (and the flush of S·S, once)
                    want = per_bin_lstsq(s, est.bounds, cols, y)
                    bins = bin_of(s, est.bounds)
                    X = np.stack(cols, axis=1).astype(np.float64)
                    fit_want = (want[bins] * X).sum(axis=1)
                    fit_beta = (beta[bins] * X).sum(axis=1)
                    assert np.abs(fit_beta - fit_want).max() <= 1e-6 * np.abs(y).max()      # the same least-squares fit, in fp64 (normal equations against QR)
                    ce = est.getConditionalExpectation(Y).getRealizations()
                    bound = (len(cols) + 2) * 2.0 ** -24 * np.abs(beta[bins] * X).sum(axis=1)
                    print(f"K={len(cols)} fusion={fusion}: max |ce - fit| / bound = {np.max(np.abs(ce - fit_beta) / bound):.3g}")
                    assert (np.abs(ce - fit_beta) <= bound).all()
                    if len(cols) > 2: continue
                    # The generic path rounds every product to fp32 (2⁻²⁴ ≈ 6e-8 relative per element) before the fp64 average.  A bin's block of
                    # {1, s} has a condition number of about (s / bin width)² <= 1e4 here, so its fit moves by at most 6e-8 · sqrt(1e4) · a small
                    # factor: 2e-4 leaves a decade.  (With s² in the basis the block's condition number is ~ 1e7 and no such bound holds: left out.)
                    with knob_off():
                        generic = gpu.MonteCarloConditionalExpectationLocalizedRegression(S, 16, basis, bounds=est.bounds)
                        beta_generic = generic.getLinearRegressionParameters(Y)
                        ce_generic = generic.getConditionalExpectation(Y).getRealizations()
                    fit_generic = (beta_generic[bins] * X).sum(axis=1)
                    print(f"knob off: max |fit - fit| = {np.abs(fit_generic - fit_beta).max():.3g}, max |ce - ce| = {np.abs(ce_generic - ce).max():.3g}")
                    assert np.abs(fit_generic - fit_beta).max() <= 2e-4 * np.abs(y).max()
                    assert np.abs(ce_generic - ce).max() <= 2e-4 * np.abs(y).max()
                # empty bins: coefficients 0, estimate 0 there
                est = gpu.MonteCarloConditionalExpectationLocalizedRegression(S, 3, [f.createRandomVariable(1.0), S], bounds=[-5.0, 100.0])
                beta = est.getLinearRegressionParameters(Y)
                assert (beta[0] == 0.0).all() and (beta[2] == 0.0).all() and beta[1].any()
        finally:
            gpu.set_fusion(prev)


def test_communicator_answers_for_the_global_sample(gpu):
    with limit(120):
        rng = np.random.default_rng(21)
        n = 40_000
        key = rng.standard_normal(n).astype(np.float32)
        data = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
        bounds = np.sort(rng.standard_normal(15))
        up = lambda a: gpu.DeviceVector.from_host(a)
        whole = gpu.binned_cross_moments(up(key), bounds, [None, up(data[0])], [up(data[1])])
        halves = [(up(key[: n // 2]), up(data[0][: n // 2]), up(data[1][: n // 2])), (up(key[n // 2:]), up(data[0][n // 2:]), up(data[1][n // 2:]))]
        local = [gpu.binned_cross_moments(h[0], bounds, [None, h[1]], [h[2]]) for h in halves]
        flat = lambda r: np.concatenate([r[0].astype(np.float64), packed(r[1], r[2]).ravel()])
        try:
            for rank in (0, 1):
                calls = []

                def gather(mine, rank=rank):
                    calls.append(mine.copy())
                    theirs = flat(local[1 - rank])
                    return np.stack([mine, theirs] if rank == 0 else [theirs, mine])

                gpu.set_expectation_comm(2, rank, gather)
                h = halves[rank]
                got = gpu.binned_cross_moments(h[0], bounds, [None, h[1]], [h[2]])
                assert len(calls) == 1 and (bits(calls[0]) == bits(flat(local[rank]))).all()       # one gather, of the local counts and sums
                assert (got[0] == whole[0]).all() and got[0].sum() == n
                assert (bits(flat(got)) == bits(flat(local[0]) + flat(local[1]))).all()            # added in rank order
                _, want, tol = exact_and_bound(key, bounds, [None, data[0]], [data[1]])
                assert (np.abs(packed(got[1], got[2]) - want) <= tol).all()
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
key = rng.standard_normal(n).astype(np.float32)
data = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
bounds = np.sort(rng.standard_normal(15))
coef = rng.standard_normal((16, 2))

def ask(k, vs):
    counts, S, T = fm.binned_cross_moments(k, bounds, [None, vs[0]], [vs[1]])
    est = fm.binned_evaluate(k, bounds, [None, vs[0]], coef)
    return {"counts": counts.tolist(), "S": S.tolist(), "T": T.tolist(), "est": est.to_float32().view(np.uint32).tolist()}

if mode == "devices":
    fm.init_devices([0, 0])
    fm.set_fusion(True)
    k = fm.DeviceVector.from_host(key); x = [fm.DeviceVector.from_host(a) for a in data]
    out = {"stored": ask(k, x), "pending": ask(k.v1s1("MULT_S", 1.0), [v.v1s1("MULT_S", 1.0) for v in x])}
    out["tiny"] = ask(fm.DeviceVector.from_host(key[:1]), [fm.DeviceVector.from_host(a[:1]) for a in data])      # shorter than the shards are many
else:
    fm.init(0)
    fm.set_thread_engines(True)
    fm.set_fusion(True)
    k = fm.DeviceVector.from_host(key); x = [fm.DeviceVector.from_host(a) for a in data]
    y = [v.v1s1("MULT_S", 1.0) for v in x]                       # pending, owned by the main thread's engine
    out = {}
    def other():
        out["stored"] = ask(k, x); out["pending"] = ask(k, y)
    t = threading.Thread(target=other); t.start(); t.join()
    out["tiny"] = ask(fm.DeviceVector.from_host(key[:1]), [fm.DeviceVector.from_host(a[:1]) for a in data])
print("RESULT " + json.dumps(out))
fm.shutdown()
'''


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """A device list {0, 0} (every shard runs the passes on its block of paths; counts add, sums add in shard order, the estimate is per
    shard) and vectors of another thread's engine, in a process of its own: the counts and the estimate of one engine exactly, the sums
    within the bound."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": root})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    rng = np.random.default_rng(31)
    n = 100_003
    key = rng.standard_normal(n).astype(np.float32)
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    bounds = np.sort(rng.standard_normal(15))
    coef = rng.standard_normal((16, 2))
    one = gpu.binned_cross_moments(gpu.DeviceVector.from_host(key), bounds, [None, gpu.DeviceVector.from_host(data[0])], [gpu.DeviceVector.from_host(data[1])])
    for name, m in (("stored", n), ("pending", n), ("tiny", 1)):
        counts, want, tol = exact_and_bound(key[:m], bounds, [None, data[0][:m]], [data[1][:m]])
        got = out[name]
        assert got["counts"] == counts.tolist(), name
        if m == n: assert got["counts"] == one[0].tolist()
        assert (np.abs(packed(np.array(got["S"]), np.array(got["T"])) - want) <= tol).all(), name
        st, est = host_evaluate(gpu, key[:m], bounds, [None, data[0][:m]], coef)
        assert np.array(got["est"], dtype=np.uint32).tolist() == est.view(np.uint32).tolist(), name


def bermudan_global_by_hand(gpu, bm, dates, basis_order):
    """The driver as it was before `bins` existed, written out against MonteCarloConditionalExpectationRegression: what bins=0 must return."""
    from test_gpu_regression import K, R, S0, SIGMA
    td = bm.getTimeDiscretization()
    x = bm.getRandomVariableForConstant(math.log(S0))
    states = []
    for i in range(len(dates)):
        x = x.add((R - 0.5 * SIGMA * SIGMA) * td.getTimeStep(i)).addProduct(bm.getBrownianIncrement(i, 0), SIGMA)
        assert abs(td.getTime(i + 1) - dates[i]) <= 1e-12
        states.append(x.exp())
    exercise_value = lambda s, date: s.bus(K).floor(0.0).div(math.exp(R * date))
    value = exercise_value(states[-1], dates[-1])
    one = bm.getRandomVariableForConstant(1.0)
    for k in range(len(dates) - 2, -1, -1):
        s = states[k]
        basis = [one, s]
        for _ in range(2, basis_order + 1): basis.append(basis[-1].mult(s))
        continuation = gpu.MonteCarloConditionalExpectationRegression(basis).getConditionalExpectation(value)
        exercise = exercise_value(s, dates[k])
        value = exercise.sub(continuation).choose(exercise, value)
    return value.getAverage()


def test_bermudan_put_localized_against_the_tree_and_the_global_fit(gpu):
    """bins=16, basis_order=1 against basis_order=5 on the same increments: at least the European value, and strictly closer to the tree.
    (A numpy restatement on the CPU gave distances of 0.2–3.6e-4 against 1.0–1.4e-3 on three seeds: a factor of three to spare.  On an MI355X:
    tree 0.153540, European 0.140139, degree 5 0.152473 (1.07e-3), 16 bins linear 0.153488 (5.3e-5), the same with the knob off.)"""
    from test_gpu_regression import K, R, S0, SIGMA, T, crr_bermudan_put, european_put
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    dates = [0.2 * k for k in range(1, 11)]
    td = gpu.TimeDiscretization(0.0, 10, 0.2)
    tree = crr_bermudan_put(dates)
    prev = gpu.set_fusion(True)
    try:
        with limit(400):
            bm = gpu.BrownianMotionHip(td, 1, 1_000_000, 31415)
            global5, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, basis_order=5)
            by_hand = bermudan_global_by_hand(gpu, bm, dates, 5)
            assert by_hand == global5 and mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, basis_order=5, bins=0)[0] == global5      # bins = 0: the global estimator's value, to the bit
            local, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, basis_order=1, bins=16)
            european = european_put(bm, T).getAverage()
            with knob_off():
                generic, _ = mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, basis_order=1, bins=16)
    finally:
        gpu.set_fusion(prev)
    print(f"tree {tree:.6f} european {european:.6f} global degree 5 {global5:.6f} (distance {abs(global5 - tree):.2e}) "
          f"16 bins linear {local:.6f} (distance {abs(local - tree):.2e}) knob off {generic:.6f}")
    assert local >= european
    assert abs(local - tree) < abs(global5 - tree), (local, global5, tree)
    assert abs(generic - local) <= 2e-4 * local                       # exercise decisions of single paths may flip
    with pytest.raises(ValueError): mc.bermudan_option_mc(bm, S0, R, SIGMA, dates, K, basis_order=3, bins=16)
