"""Kernel regression on the device (include/fmhip.h: fmhip_kernel_moments; csrc/kreg_kernel.hip) on a real MI355X: the device
sums EQUAL the host definition's bit for bit on dyadic data at every size and slicing, the uniform kernel's W equals the member counts of
fmhip_count_not_above (an independent kernel), random data with edge keys lie within the derived bound, one (point, entry) sum keeps its
bits whatever else the call names, the frame (one launch, one flush, the refusals, the knob-off path), the estimator, a device list, thread
engines and a two-rank communicator, and the local-stochastic-volatility driver end to end against Black–Scholes.

Every test prints the figures it asserts on before it asserts (run with -s).  No test asks the device for anything out of range: bad
arguments are refused on the host before a launch."""
import json
import math
import os
import signal
import subprocess
import sys
from importlib import import_module

import numpy as np
import pytest

from test_kernel_regression_cpu import GRID, KERNELS, bits, bound, dyadic_case, edge_grid, edge_keys, numpy_moments, terms_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 255, 1024, 1025, 256 * 1024 + 1, 2 ** 20 + 3]      # the tile's edge, more tiles than workgroups (256 x 1024 + 1), a ragged tail
POINTS = [1, 2, 36, 37, 256]                                    # 36 -> 37 crosses the slice edge at 2 entries per point


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
        self.prev = os.environ.get("FMHIP_DEVICE_KERNEL_MOMENTS")
        os.environ["FMHIP_DEVICE_KERNEL_MOMENTS"] = "0"
    def __exit__(self, *a):
        if self.prev is None: del os.environ["FMHIP_DEVICE_KERNEL_MOMENTS"]
        else: os.environ["FMHIP_DEVICE_KERNEL_MOMENTS"] = self.prev


def slices(Q, order, n_y):
    qe = 1 + n_y if order == 0 else 3 + 2 * n_y
    per = min(Q, 72 // qe)
    return -(-Q // per)


def up(gpu, a): return gpu.DeviceVector.from_host(np.ascontiguousarray(a, dtype=np.float32))


def exact_in_any_order(key, points, h, ys, kernel, order):
    """members x max|term| / GRID < 2⁵³ at the fullest point, every term on the grid: the device's tree and the definition's path order add
    the same exact numbers without a rounding."""
    xd = key.astype(np.float64)
    with np.errstate(invalid="ignore"):
        counts = [int(((p - h < xd) & (xd < p + h)).sum()) for p in points[:: max(len(points) // 16, 1)]]
    q = int(np.argmax(counts)) * max(len(points) // 16, 1)
    m, terms = terms_of(key, points, h, ys, kernel, order, q)
    for t in terms:
        if t.size == 0: continue
        assert (t / GRID == np.rint(t / GRID)).all() and float(np.abs(t).max()) * t.size / GRID < 2.0 ** 53


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_definition_on_dyadic_data(gpu, n):
    """Keys k/8, points on multiples of 1/4, dyadic bandwidths, integer |y| <= 16: every sum is exact in any order, so the device's sums are
    the definition's bit for bit — sliced and unsliced, both orders, 0 / 1 / 4 dependents."""
    large = n >= 2 ** 18
    shapes = [(0, 1), (1, 4)] if large else [(0, 0), (0, 1), (0, 4), (1, 0), (1, 1), (1, 4)]
    seen = set()
    with limit(240):
        for Q in ([36, 37, 256] if large else POINTS):
            for order, n_y in shapes:
                kernel = KERNELS[(Q + order + n_y) % 5]
                h = 0.5 if kernel == "triweight" or large else [0.5, 1.0, 2.0][(Q + n_y) % 3]
                key, points, h, ys = dyadic_case(n, Q, h, seed=n % 1000 + Q, n_y=n_y)
                if n > 8: key[[2, 3, 4, 5]] = [np.nan, np.inf, -np.inf, -0.0]
                exact_in_any_order(key, points, h, ys, kernel, order)
                K, Y = up(gpu, key), [up(gpu, y) for y in ys]
                before = gpu.pool_stats().n_kernel_launches
                got = gpu.kernel_moments(K, points, h, Y, kernel, order)
                assert gpu.pool_stats().n_kernel_launches - before == 1
                want = gpu.kernel_moments_host(key, points, h, ys, kernel, order)
                differ = np.argwhere(bits(got) != bits(want))
                assert differ.size == 0, (n, Q, order, n_y, kernel, differ[:4], got[tuple(differ[0])], want[tuple(differ[0])])
                seen.add(slices(Q, order, n_y))
    print(f"n={n}: slice counts exercised {sorted(seen)}")
    assert 1 in seen and max(seen) > 1


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_kernel_at_one_shape(gpu, kernel):
    with limit(120):
        for order in (0, 1):
            key, points, h, ys = dyadic_case(4099, 37, 0.5 if kernel == "triweight" else 1.0, seed=17, n_y=2)
            exact_in_any_order(key, points, h, ys, kernel, order)
            got = gpu.kernel_moments(up(gpu, key), points, h, [up(gpu, y) for y in ys], kernel, order)
            assert (bits(got) == bits(gpu.kernel_moments_host(key, points, h, ys, kernel, order))).all(), (kernel, order)


def test_uniform_weights_equal_the_counts_of_an_independent_kernel(gpu):
    """W_q of the uniform kernel is the number of members; kernel_counts takes it from fmhip_count_not_above: #{x <= pred(upper)} − #{x <= lower}."""
    rng = np.random.default_rng(41)
    n = 2 ** 20 + 3
    key = rng.standard_normal(n).astype(np.float32)
    points = np.linspace(-4.0, 4.0, 256)
    h = 0.1 + 0.02 * np.abs(points)                                 # widening in the tails, slowly enough
    points[7] = float(key[11]) + h[7]; points = np.sort(points)     # a key exactly on a lower end …
    h = 0.1 + 0.02 * np.abs(points)
    key[12] = np.float32(points[100] + h[100])                      # … (nearly) on an upper end, and the edge inputs
    key[:6] = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45]
    with limit(120):
        K = up(gpu, key)
        W = gpu.kernel_moments(K, points, h, (), "uniform", 0)[:, 0]
        counts = gpu.kernel_counts(K, points, h)
    xd = key.astype(np.float64)
    with np.errstate(invalid="ignore"):
        members = np.array([int(((p - b < xd) & (xd < p + b)).sum()) for p, b in zip(points, h)])
    print(f"members per point: {members.min()} … {members.max()}")
    assert (W == counts).all() and (counts == members).all()


def test_random_data_within_the_derived_bound(gpu):
    """|device − definition| <= 2·m_q·2⁻⁵³·Σ|terms|·(1 + 1e-6) per (q, entry): two summation orders of the same exact fp64 terms.  Edge keys, keys
    exactly on lower_q and upper_q, and a y that is NaN inside one support: the points that hold it are NaN, every other point is compared."""
    rng = np.random.default_rng(43)
    n = 256 * 1024 + 1
    points = np.sort(np.concatenate([edge_grid()[0], np.linspace(-3.0, 5.0, 53)]))      # duplicated points among them
    h = 0.25 + np.abs(points - 1.0) / 16.0                          # a bandwidth per point; |dh/dp| < 1: lower and upper stay monotone; dyadic where p is
    assert points.size == 64 and (np.diff(points - h) >= 0).all() and (np.diff(points + h) >= 0).all()
    key = rng.standard_normal(n).astype(np.float32) * np.float32(1.5) + np.float32(0.5)
    edges = edge_keys(points, h)
    key[100:100 + edges.size] = edges
    xd = key.astype(np.float64)
    assert (xd[:, None] == (points - h)[None, :]).any() and (xd[:, None] == (points + h)[None, :]).any()      # keys exactly ON a lower and an upper end
    y0 = rng.standard_normal(n).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"): y1 = (2 + 3 * key).astype(np.float32)      # the edge keys overflow: replaced below
    poisoned = 5000
    key[poisoned] = np.float32(-2.9); y0[poisoned] = np.nan         # inside the supports of the leftmost points only
    y1[~np.isfinite(y1)] = 1.0
    with limit(120):
        K, Y0, Y1 = up(gpu, key), up(gpu, y0), up(gpu, y1)
        for order in (0, 1):
            got = gpu.kernel_moments(K, points, h, [Y0, Y1], "epanechnikov", order)
            want = gpu.kernel_moments_host(key, points, h, [y0, y1], "epanechnikov", order)
            _, absolute, members = numpy_moments(key, points, h, [y0, y1], "epanechnikov", order)
            holds = (points - h < -2.9) & (-2.9 < points + h)        # float32(-2.9) lies strictly inside or outside every support of this grid
            assert np.isclose(np.abs(points - h + 2.9), 0, atol=1e-6).sum() == 0 and np.isclose(np.abs(points + h + 2.9), 0, atol=1e-6).sum() == 0
            y0_entries = [1] if order == 0 else [3, 5]
            clean = np.ones_like(got, dtype=bool); clean[np.ix_(holds, y0_entries)] = False
            assert 0 < holds.sum() <= 6 and (~holds).sum() >= 0.9 * points.size
            assert np.isnan(got[~clean]).all() and np.isnan(want[~clean]).all()
            assert np.isfinite(got[clean]).all()
            err, tol = np.abs(got - want), bound(absolute, members)
            worst = np.max(err[clean] / np.maximum(tol[clean], 1e-300))
            print(f"order {order}: {int(clean.sum())} of {clean.size} sums compared, members {members.min()} … {members.max()}, max |device - definition| / bound = {worst:.3g}")
            assert (err[clean] <= tol[clean]).all()
        with knob_off():                                             # the knob-off path: the same layout, the definition's bits
            off = gpu.kernel_moments(K, points, h, [Y0, Y1], "epanechnikov", 1)
        assert off.shape == got.shape and (bits(off)[clean] == bits(want)[clean]).all() and np.isnan(off[~clean]).all()


def test_a_sum_keeps_its_bits_whatever_else_the_call_names(gpu):
    """One (point, entry) sum is a function of n, of which positions are members and of the values there: the same bits with 2 points or 256,
    with more or fewer dependents, for order 0 or 1, with y in another slot, in a call of 1 slice or 43."""
    rng = np.random.default_rng(47)
    n = 256 * 1024 + 1
    key = rng.standard_normal(n).astype(np.float32)
    ys = [rng.standard_normal(n).astype(np.float32) for _ in range(4)]
    many = np.linspace(-3.0, 3.0, 256)
    a, b = 40, 200
    two, h = many[[a, b]], 0.35
    with limit(120):
        K, Y = up(gpu, key), [up(gpu, y) for y in ys]
        base0 = gpu.kernel_moments(K, two, h, [Y[0]], "quartic", 0)                  # [W, Wy0], 1 slice
        base1 = gpu.kernel_moments(K, two, h, [Y[0]], "quartic", 1)                  # [W, Wd, Wdd, Wy0, Wdy0], 1 slice
        wide0 = gpu.kernel_moments(K, many, h, [Y[1], Y[2], Y[0], Y[3]], "quartic", 0)[[a, b]]      # 256 points x 5 entries: 19 slices, y0 in slot 2
        wide1 = gpu.kernel_moments(K, many, h, [Y[1], Y[2], Y[0], Y[3]], "quartic", 1)[[a, b]]      # 256 points x 11 entries: 43 slices
        bare = gpu.kernel_moments(K, many, h, (), "quartic", 0)[[a, b]]              # 256 points x 1 entry: 4 slices
    assert slices(2, 0, 1) == 1 and slices(256, 0, 4) == 19 and slices(256, 1, 4) == 43 and slices(256, 0, 0) == 4
    for other in (base1[:, 0], wide0[:, 0], wide1[:, 0], bare[:, 0]): assert (bits(other) == bits(base0[:, 0])).all()       # W
    for other in (base1[:, 3], wide0[:, 3], wide1[:, 5]): assert (bits(other) == bits(base0[:, 1])).all()                   # W·y0
    assert (bits(wide1[:, 1:3]) == bits(base1[:, 1:3])).all() and (bits(wide1[:, 9]) == bits(base1[:, 4])).all()            # Wd, Wdd, Wd·y0
    assert (base0[:, 0] > 0).all()


def test_frame(gpu):
    """One launch per call; pending inputs cost what ONE flush of them costs; a given-up vector, a size mismatch and a foreign handle are the
    errors the other passes answer; nothing is refused late."""
    N = gpu._native
    rng = np.random.default_rng(53)
    n = 100_003
    key, y = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    points, h = np.linspace(-2, 2, 37), 0.3
    prev = gpu.set_fusion(True)
    try:
        with limit(120):
            K, Y = up(gpu, key), up(gpu, y)
            launches = lambda: gpu.pool_stats().n_kernel_launches
            want = gpu.kernel_moments(up(gpu, key * np.float32(2.0)), points, h, [up(gpu, y * np.float32(2.0))], "epanechnikov", 1)
            pk, py = K.v1s1("MULT_S", 2.0), Y.v1s1("MULT_S", 2.0)
            t0 = launches(); gpu.flush(); flush_cost = launches() - t0
            pk2, py2 = K.v1s1("MULT_S", 2.0), Y.v1s1("MULT_S", 2.0)
            t0 = launches()
            got = gpu.kernel_moments(pk2, points, h, [py2], "epanechnikov", 1)     # pending expressions: one flush, then the pass
            cost = launches() - t0
            print(f"a flush of the two pending operands: {flush_cost} launches; the call on pending operands: {cost}")
            assert cost == flush_cost + 1 and flush_cost >= 1
            assert (bits(got) == bits(want)).all()
            t0 = launches(); gpu.kernel_moments(pk, points, h, [py], "epanechnikov", 1); assert launches() - t0 == 1
            base = up(gpu, np.arange(4096, dtype=np.float32))
            ys = [base.v1s1("ADD_S", float(k)) for k in range(1, 5)]
            gpu.give_up_values(ys)
            gpu.reduce_moments_batch_end(gpu.reduce_moments_batch_begin(ys), len(ys))
            for k, v in enumerate(ys, start=1):
                try:
                    s = gpu.kernel_moments(base, [2048.0], 4096.0, [v], "uniform", 0)
                    assert s[0, 0] == 4096 and s[0, 1] == 4096 * 4095 / 2 + 4096 * k
                except gpu.FmhipError as e:
                    assert e.code == N.ERR_INVALID_ARGUMENT and "given up" in str(e)
            t0 = launches()
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, [0.0, 1.0, 0.5], h, [Y])
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, [0.0, 1.0], [1.0, 2.5], [Y])
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, points, h, [Y], "epanechnikov", 2)
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, np.zeros(257), h, [Y])
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, points, h, [Y] * 5)
            assert e.value.code == N.ERR_INVALID_ARGUMENT
            with pytest.raises(gpu.FmhipError) as e: gpu.kernel_moments(K, points, h, [up(gpu, y[:-1])])
            assert e.value.code == N.ERR_SIZE_MISMATCH
            out = np.zeros(37 * 2); hy = (N.C.c_int64 * 1)(K.handle + (1 << 30)); PD = N.C.POINTER(N.C.c_double)
            st = gpu.lib().fmhip_kernel_moments(K.handle, points.ctypes.data_as(PD), np.full(37, h).ctypes.data_as(PD), 37, 2, 0, hy, 1, out.ctypes.data_as(PD))
            assert st == N.ERR_INVALID_HANDLE
            assert launches() == t0                                  # refused on the host: nothing was launched
    finally:
        gpu.set_fusion(prev)


def test_estimator(gpu):
    """y = 2 + 3x with order 1: the fitted values are the line within the rounding of the solve; getConditionalExpectation is two launches
    and equals table_apply_host of the fitted values bit for bit; the kernel density of a large normal sample integrates to 1 within the
    quadrature error of the grid."""
    rng = np.random.default_rng(59)
    n = 2 ** 20
    x = (rng.integers(-4 * 4096, 4 * 4096 + 1, n) / 4096.0).astype(np.float32)      # on a grid of 2⁻¹²: y = 2 + 3x is an fp32 number, ON the line
    y = (2.0 + 3.0 * x).astype(np.float32)
    assert (y.astype(np.float64) == 2.0 + 3.0 * x.astype(np.float64)).all()
    points = np.linspace(-3.5, 3.5, 64)
    with limit(120):
        X, Y = gpu.RandomVariableHip(0.0, up(gpu, x)), gpu.RandomVariableHip(0.0, up(gpu, y))
        est = gpu.MonteCarloConditionalExpectationKernelRegression(X, points, 0.25, "epanechnikov", order=1)
        fitted = est.getFittedValues(Y)
        # the sums carry m·2⁻⁵³ relative each (m <= 2¹⁷ members: 2⁻³⁶); the solve divides by det = W·Wdd − Wd² >= W·Wdd/2 for these windows
        # (uniform keys: Wd² << W·Wdd) and |Wy| <= 13·W: 13·8·2⁻³⁶ < 2e-9
        print(f"order 1 on the line: max |fitted - line| = {np.abs(fitted - (2.0 + 3.0 * points)).max():.3g}")
        assert np.abs(fitted - (2.0 + 3.0 * points)).max() <= 2e-9
        before = gpu.pool_stats().n_kernel_launches
        ce = est.getConditionalExpectation(Y)
        got = ce.realizations.to_float32()
        assert gpu.pool_stats().n_kernel_launches - before == 2      # one moments launch, one table launch
        table = gpu.TabulatedFunction(points, fitted, "linear", "constant")
        assert (got.view(np.uint32) == gpu.table_apply_host(x, [table])[0].view(np.uint32)).all()
        inside = np.abs(x) <= 3.5
        assert np.abs(got[inside].astype(np.float64) - y[inside]).max() <= 2e-6      # fp32 narrowing of values up to 12.5
        # density: uniform grid of spacing D, h = 8 D.  Σ_q f(p_q)·D is the rectangle rule on every kernel bump K_h(· − x_i), a quadratic with a
        # kink at both ends of its support: Euler–Maclaurin gives |error| <= D²/12·Σ|jump K'| + D³/6·max|B₃|·Σ|jump K''| = D²/(4h²) + 0.0241·D³/h³.
        z = rng.standard_normal(n).astype(np.float32)
        grid = np.linspace(-7.0, 7.0, 256); D = grid[1] - grid[0]; h = 8 * D
        assert np.abs(z).max() + h < 7.0
        density = gpu.kernel_density(gpu.RandomVariableHip(0.0, up(gpu, z)), grid, h, "epanechnikov")
    integral = float(density.sum() * D)
    quadrature = D ** 2 / (4 * h ** 2) + 0.0241 * D ** 3 / h ** 3
    print(f"kernel density: integral {integral:.9f}, quadrature bound {quadrature:.3g}")
    assert abs(integral - 1.0) <= quadrature + 1e-12
    phi = np.exp(-0.5 * grid ** 2) / math.sqrt(2 * math.pi)
    assert np.abs(density - phi).max() <= h ** 2 / 2 * 0.4 / 5 + 5 * math.sqrt(0.4 * 0.6 / (n * h))      # bias h²/2·μ₂·|φ''| and five standard errors


def test_communicator_answers_for_the_global_sample(gpu):
    with limit(120):
        rng = np.random.default_rng(61)
        n = 40_000
        key = rng.standard_normal(n).astype(np.float32)
        y = rng.standard_normal(n).astype(np.float32)
        points, h = np.linspace(-2.5, 2.5, 40), 0.3
        ask = lambda k, v: gpu.kernel_moments(up(gpu, k), points, h, [up(gpu, v)], "triangular", 1)
        local = [ask(key[: n // 2], y[: n // 2]), ask(key[n // 2:], y[n // 2:])]
        try:
            for rank in (0, 1):
                calls = []

                def gather(mine, rank=rank):
                    calls.append(mine.copy())
                    theirs = local[1 - rank].ravel()
                    return np.stack([mine, theirs] if rank == 0 else [theirs, mine])

                gpu.set_expectation_comm(2, rank, gather)
                half = slice(0, n // 2) if rank == 0 else slice(n // 2, n)
                got = ask(key[half], y[half])
                assert len(calls) == 1 and (bits(calls[0]) == bits(local[rank].ravel())).all()      # ONE gather, of the local sums
                assert (bits(got) == bits(local[0] + local[1])).all()                               # added in rank order
        finally:
            gpu.set_expectation_comm(1, 0, None)
        _, absolute, members = numpy_moments(key, points, h, [y], "triangular", 1)
        want = gpu.kernel_moments_host(key, points, h, [y], "triangular", 1)
        assert (np.abs(got - want) <= bound(absolute, members)).all()


_OTHER_MODES = r'''
import importlib, json, sys, threading
import numpy as np
sys.path.insert(0, %(root)r)
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
mode = sys.argv[1]
rng = np.random.default_rng(67)
n = 100_003
key = rng.standard_normal(n).astype(np.float32)
data = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
points = np.linspace(-2.5, 2.5, 40)

def ask(k, vs):
    return fm.kernel_moments(k, points, 0.3, vs, "epanechnikov", 1).view(np.uint64).ravel().tolist()      # 40 x 7 entries: 4 slices

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


def shard_range(n, shards, shard):
    """csrc/sharded.cpp: blocks of whole 16-byte groups."""
    groups = (n + 3) // 4
    base, extra = divmod(groups, shards)
    g0 = shard * base + min(shard, extra); g1 = g0 + base + (1 if shard < extra else 0)
    return min(g0 * 4, n), min(g1 * 4, n)


@pytest.mark.parametrize("mode", ["devices", "threads"])
def test_device_list_and_thread_engines(gpu, mode, tmp_path):
    """A device list {0, 0} (every shard runs the pass on its block of paths; the sums add in shard order: bit for bit the sum of the parts)
    and vectors of another thread's engine (one engine's bits), in a process of its own."""
    script = tmp_path / "modes.py"
    script.write_text(_OTHER_MODES % {"root": ROOT})
    r = subprocess.run([sys.executable, str(script), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    rng = np.random.default_rng(67)
    n = 100_003
    key = rng.standard_normal(n).astype(np.float32)
    data = [rng.standard_normal(n).astype(np.float32) for _ in range(2)]
    points = np.linspace(-2.5, 2.5, 40)
    with limit(120):
        def one(lo, hi): return gpu.kernel_moments(up(gpu, key[lo:hi]), points, 0.3, [up(gpu, a[lo:hi]) for a in data], "epanechnikov", 1)
        for name, m in (("stored", n), ("pending", n), ("tiny", 1)):
            if mode == "devices":
                parts = [one(*shard_range(m, 2, d)) for d in (0, 1) if shard_range(m, 2, d)[1] > shard_range(m, 2, d)[0]]
                want = parts[0] if len(parts) == 1 else parts[0] + parts[1]
            else: want = one(0, m)
            assert np.array(out[name], dtype=np.uint64).tolist() == bits(want).ravel().tolist(), (mode, name)


# ---------------------------------------------------------------- local-stochastic volatility, end to end
S0, R, T, SIGMA = 100.0, 0.05, 1.0, 0.2
V0, KAPPA, THETA, XI, RHO = 0.09, 1.5, 0.04, 0.5, -0.5
STRIKES = (80.0, 100.0, 120.0)
SURFACE = dict(times=[0.0], spots=[50.0, 100.0, 200.0], dupire_vols=[[SIGMA, SIGMA, SIGMA]])


def test_local_stochastic_volatility_reprices_the_dupire_surface(gpu):
    """2¹⁶ paths, 50 steps, T = 1, S0 = 100, r = 0.05, a flat Dupire volatility of 0.2 under Heston's variance (v0 = 0.09, κ = 1.5, θ = 0.04,
    ξ = 0.5, ρ = −0.5): the particle method's leverage makes the model reprice Black–Scholes(σ = 0.2).  Each price within 3 standard errors of
    the closed form and at most a quarter as far from it as the same run with the leverage fixed at 1 (heston_call_mc on the same
    increments).  A numpy prototype of this scheme (another generator) gave 0.66, −0.20, −0.91 standard errors at order 0 and 0.42, −0.47,
    −1.01 at order 1, the unleveraged run off by 17 to 28.
    Measured on an MI355X (seed 31415), in standard errors: order 0: K = 80 −0.92, K = 100 −0.96, K = 120 −1.71; order 1: −1.15, −1.23, −1.83;
    leverage 1: +18.6, +28.2, +17.8 (distance ratios 0.034 … 0.102).  The oracle's fp32 classes fed with the same increments give the same
    figures to the digits shown.  The bias is the scheme's (50 Euler steps, local-constant smoothing over 3 Silverman bandwidths): at 10⁶
    paths K = 100 is 10.4174 ± 0.0147 against 10.4506, −2.3 standard errors — do not test there with this step count.
    With ξ = 0 the variance is deterministic, E[v | S] = v, and the model IS the local-volatility model of the surface: within 3 standard
    errors of local_volatility_call_mc on the same increments (measured: 10.466298 for both)."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = gpu.TimeDiscretization(0.0, 50, T / 50)
    prev = gpu.set_fusion(True)
    try:
        with limit(400):
            bm = gpu.BrownianMotionHip(td, 2, 2 ** 16, 31415)
            rows = []
            for K in STRIKES:
                exact = mc.black_scholes_call_analytic(S0, R, SIGMA, T, K)
                plain = mc.heston_call_mc(bm, S0, R, V0, KAPPA, THETA, XI, RHO, T, K)[0]
                rows.append((K, exact, plain, [mc.stochastic_local_volatility_call_mc(bm, S0, R, **SURFACE, v0=V0, kappa=KAPPA, theta=THETA, xi=XI, rho=RHO, maturity=T, strike=K, order=order)
                                               for order in (0, 1)]))
            flat = mc.stochastic_local_volatility_call_mc(bm, S0, R, **SURFACE, v0=V0, kappa=KAPPA, theta=THETA, xi=0.0, rho=RHO, maturity=T, strike=100.0)
            local = mc.local_volatility_call_mc(bm, S0, R, SURFACE["times"], SURFACE["spots"], SURFACE["dupire_vols"], T, 100.0)
    finally:
        gpu.set_fusion(prev)
    for K, exact, plain, runs in rows:
        for order, (value, se) in enumerate(runs):
            print(f"K={K:.0f} order {order}: {value:.5f} against {exact:.5f}: {(value - exact) / se:+.2f} standard errors (se {se:.5f}); leverage 1: {plain:.5f}, {(plain - exact) / se:+.2f}")
    print(f"xi = 0: {flat[0]:.6f} ± {flat[1]:.6f}, local volatility {local[0]:.6f}")
    for K, exact, plain, runs in rows:
        for value, se in runs:
            assert abs(value - exact) <= 3.0 * se, (K, value, exact, se)
            assert abs(value - exact) <= 0.25 * abs(plain - exact), (K, value, plain, exact)
    assert abs(flat[0] - local[0]) <= 3.0 * flat[1]
