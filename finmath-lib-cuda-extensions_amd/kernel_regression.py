"""Kernel regression on the device (include/fmhip.h: fmhip_kernel_moments, fmhip_kernel_moments_host): E[y | x = p_q] at
a grid of points p_q by kernel weights — the conditional expectation AS A CURVE: the inner step of the particle method for
local-stochastic-volatility calibration (Guyon, Henry-Labordère: E[v_t | S_t = S] at every time step), kernel density estimates, smooth
exercise boundaries, exposure profiles.  One launch returns the kernel-weighted local moments of up to four vectors at up to 256 points;
TabulatedFunction (tabulated.py) turns the fitted values at the points back into a vector on the device.

The definition is host/kernel_regression.hpp, one header that the host and the kernel both compile: lower = p − h, upper = p + h, a member
of point q is an element with lower_q < (double)key < upper_q, its weight 1 | 1 − |u| | t | t² | t³ with u = (key − p)/h, t = 1 − u², the
sums [w, w·y…] (order 0) or [w, w·d, w·d², w·y…, w·d·y…] (order 1) in fp64.  kernel_local_fit makes the local constant or local linear
fit of them; a point without members is filled from its fitted neighbours.

FMHIP_DEVICE_KERNEL_MOMENTS=0, read per call: the A/B switch and the fallback — the vectors are downloaded and fmhip_kernel_moments_host
(the definition) runs on one core.  A key that is no RandomVariableHip (any other RandomVariable class) always takes that path.  The
device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip, select_ranks_batch
from .tabulated import TabulatedFunction, table_apply_host

MAX_POINTS, MAX_Y = 256, 4                                   # fmhip_kernel_moments' limits
KERNELS = {"uniform": 0, "triangular": 1, "epanechnikov": 2, "quartic": 3, "triweight": 4}
# ∫ K = 1 on [−1, 1] for c_K · w(u)
NORMALISATION = {"uniform": 0.5, "triangular": 1.0, "epanechnikov": 0.75, "quartic": 15.0 / 16.0, "triweight": 35.0 / 32.0}
FIT_TOLERANCE = 1e-12                                        # local linear: det <= this · W · Wdd falls back to the local constant

_pd = C.POINTER(C.c_double)


def device_kernel_moments() -> bool:
    """FMHIP_DEVICE_KERNEL_MOMENTS=0: kernel_moments downloads the vectors and runs the definition on the host (the A/B switch and the
    fallback); anything else: one fmhip_kernel_moments launch.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_KERNEL_MOMENTS", "1") != "0"


def entries_per_point(order: int, n_y: int) -> int:
    return 1 + n_y if order == 0 else 3 + 2 * n_y


def _kernel(kernel) -> int:
    if isinstance(kernel, str):
        if kernel not in KERNELS: raise ValueError(f"kernel {kernel!r} (one of {sorted(KERNELS)})")
        return KERNELS[kernel]
    return int(kernel)


def _grid(points, bandwidths):
    p = np.ascontiguousarray(points, dtype=np.float64).ravel()
    h = np.asarray(bandwidths, dtype=np.float64)
    h = np.ascontiguousarray(np.broadcast_to(h, p.shape) if h.ndim == 0 else h.ravel())
    if h.size != p.size: raise ValueError(f"{p.size} points and {h.size} bandwidths")
    return p, h


def _vector(v):
    """The device vector behind v, or None if v lives elsewhere."""
    if isinstance(v, RandomVariableHip):
        if v.isDeterministic(): raise ValueError("a deterministic random variable has no vector")
        return v.realizations
    return v if isinstance(v, DeviceVector) else None


def _host_values(v) -> np.ndarray:
    d = _vector(v) if isinstance(v, (RandomVariableHip, DeviceVector)) else None
    if d is not None: return d.to_float32()
    if hasattr(v, "getRealizations"):
        if v.isDeterministic(): raise ValueError("a deterministic random variable has no vector")
        return np.ascontiguousarray(v.getRealizations(), dtype=np.float32)
    return np.ascontiguousarray(v, dtype=np.float32).ravel()


def kernel_moments_host(key, points, bandwidths, y=(), kernel="epanechnikov", order=0) -> np.ndarray:
    """The DEFINITION (fmhip_kernel_moments_host) over host arrays: [Q, entries] float64; needs no device."""
    p, h = _grid(points, bandwidths)
    k = np.ascontiguousarray(key, dtype=np.float32).ravel()
    ys = [np.ascontiguousarray(v, dtype=np.float32).ravel() for v in y]
    out = np.empty((p.size, entries_per_point(int(order), len(ys))), dtype=np.float64)
    cols = (C.c_void_p * max(len(ys), 1))(*[v.ctypes.data for v in ys])
    for v in ys:
        if v.size != k.size: raise N.FmhipError(N.ERR_SIZE_MISMATCH, "kernel moments over vectors of different size")
    N.check(N.lib().fmhip_kernel_moments_host(k.ctypes.data_as(C.c_void_p), k.size, p.ctypes.data_as(_pd), h.ctypes.data_as(_pd), p.size, _kernel(kernel), int(order),
                                              cols if ys else None, len(ys), out.ctypes.data_as(_pd)))
    return out


def kernel_moments(key, points, bandwidths, y=(), kernel="epanechnikov", order=0) -> np.ndarray:
    """sums[Q, entries] (float64) of the kernel-weighted local moments of the vectors y (0 … 4) at the points of `key`, from ONE device launch:
    order 0: [W, Wy_0, …]; order 1: [W, Wd, Wdd, Wy_0, …, Wdy_0, …], d = key − p_q.  `bandwidths`: one number or one per point; lower = p − h
    and upper = p + h must both be non-decreasing.  Sums, not averages: the normalisation is the caller's."""
    ys = list(y)
    dk = _vector(key)
    dys = [_vector(v) for v in ys]
    if not device_kernel_moments() or dk is None or any(d is None for d in dys):
        return kernel_moments_host(_host_values(key), points, bandwidths, [_host_values(v) for v in ys], kernel, order)
    p, h = _grid(points, bandwidths)
    out = np.empty((p.size, entries_per_point(int(order), len(ys))), dtype=np.float64)
    hy = (C.c_int64 * max(len(ys), 1))(*[d.handle for d in dys])
    N.check(N.lib().fmhip_kernel_moments(dk.handle, p.ctypes.data_as(_pd), h.ctypes.data_as(_pd), p.size, _kernel(kernel), int(order), hy if ys else None, len(ys),
                                         out.ctypes.data_as(_pd)))
    return out


def kernel_counts(key, points, bandwidths) -> np.ndarray:
    """Members per point (int64): #{ x <= pred(upper_q) } − #{ x <= lower_q }, from the EXISTING fmhip_count_not_above — for minimum-count
    policies, and an independent cross-check of the uniform kernel's W."""
    p, h = _grid(points, bandwidths)
    edges = np.concatenate([np.nextafter(p + h, -np.inf), p - h])
    d = _vector(key)
    if d is not None: c = d.count_not_above(edges)
    else:
        x = _host_values(key).astype(np.float64)
        c = np.array([np.count_nonzero(x <= e) for e in edges], dtype=np.int64)
    return c[:p.size] - c[p.size:]


def _sample_size(key) -> int:
    if isinstance(key, RandomVariableHip): return key._sample_size()
    if isinstance(key, DeviceVector): return RandomVariableHip(0.0, key)._sample_size()
    return int(key.size()) if hasattr(key, "size") and callable(key.size) else int(np.size(key))


def silverman_bandwidth(key, factor: float = 1.0) -> float:
    """Silverman's rule of thumb: 1.06 · σ · n^(−1/5) · factor, σ² = getVariance()."""
    rv = RandomVariableHip(0.0, key) if isinstance(key, DeviceVector) else key
    n = _sample_size(key)
    return 1.06 * math.sqrt(rv.getVariance()) * n ** -0.2 * float(factor)


def kernel_density(key, points, bandwidths, kernel="epanechnikov") -> np.ndarray:
    """The kernel density estimate at the points: W_q · c_K / (n · h_q)."""
    p, h = _grid(points, bandwidths)
    name = kernel if isinstance(kernel, str) else {v: k for k, v in KERNELS.items()}[int(kernel)]
    W = kernel_moments(key, p, h, (), kernel, 0)[:, 0]
    return W * NORMALISATION[name] / (_sample_size(key) * h)


def kernel_local_fit(sums, order: int, n_y: int, points):
    """(values, slopes), each [n_y, Q], from sums[Q, entries] (host/kernel_regression.hpp: kernel_local_fit).  Order 0: Wy / W, slope 0.
    Order 1: the 2×2 solve of [[W, Wd], [Wd, Wdd]], and order 0 where the determinant is not above 1e-12 · W · Wdd.  A point with W == 0 has
    no fit: it is filled by linear interpolation in p between its nearest fitted neighbours, or by the nearest one's value beyond the
    outermost fitted points.  No fitted point at all: ValueError."""
    s = np.asarray(sums, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64).ravel()
    Q = p.size
    s = s.reshape(Q, entries_per_point(order, n_y))
    if n_y < 1: raise ValueError("a fit needs a dependent")
    W = s[:, 0]
    fitted = (W > 0.0) & np.isfinite(W)
    if not fitted.any(): raise ValueError("kernel fit: no point has a member with a positive weight")
    values, slopes = np.zeros((n_y, Q)), np.zeros((n_y, Q))
    with np.errstate(all="ignore"):
        for m in range(n_y):
            if order == 0:
                values[m] = np.where(fitted, s[:, 1 + m] / W, 0.0)
                continue
            Wd, Wdd, Wy, Wdy = s[:, 1], s[:, 2], s[:, 3 + m], s[:, 3 + n_y + m]
            det = W * Wdd - Wd * Wd
            linear = fitted & (det > FIT_TOLERANCE * W * Wdd)
            values[m] = np.where(linear, (Wdd * Wy - Wd * Wdy) / det, np.where(fitted, Wy / W, 0.0))
            slopes[m] = np.where(linear, (W * Wdy - Wd * Wy) / det, 0.0)
    at = np.flatnonzero(fitted)
    for q in np.flatnonzero(~fitted):
        left, right = at[at < q], at[at > q]
        l, r = (left[-1] if left.size else -1), (right[0] if right.size else -1)
        for a in (values, slopes):
            if l >= 0 and r >= 0 and p[r] > p[l]:
                f = (p[q] - p[l]) / (p[r] - p[l])
                a[:, q] = a[:, l] + f * (a[:, r] - a[:, l])
            else: a[:, q] = a[:, l if l >= 0 else r]
    return values, slopes


def default_points(key, n_points: int = 64) -> np.ndarray:
    """n_points uniform between the 0.1 % and the 99.9 % quantile of the key: ONE select_ranks_batch call on the device."""
    n = _sample_size(key)
    ranks = [int(math.floor(0.001 * (n - 1))), int(math.ceil(0.999 * (n - 1)))]
    d = _vector(key)
    if d is not None: lo, hi = select_ranks_batch([d], ranks)[0]
    else:
        s = np.sort(_host_values(key).astype(np.float64))
        lo, hi = s[ranks[0]], s[ranks[1]]
    return np.linspace(float(lo), float(hi), int(n_points))


class MonteCarloConditionalExpectationKernelRegression:
    """E[ · | key] by kernel regression at a grid of points of `key`, interpolated between them: local constant (order 0,
    Nadaraya–Watson) or local linear (order 1) fits with a compactly supported kernel.  points: the grid (None or an int: that many —
    64 — uniform between the 0.1 % and 99.9 % quantiles of the key); bandwidths: one number or one per point (None: max(3 · Silverman,
    1.5 · spacing)).  getFittedValues: one moments launch per four dependents; getConditionalExpectation: that, and one
    TabulatedFunction launch per dependent (constant extrapolation beyond the outermost points)."""

    def __init__(self, key, points=None, bandwidths=None, kernel="epanechnikov", order=1, interpolation="linear"):
        if key.isDeterministic(): raise ValueError("the key of a kernel regression is a stochastic random variable")
        if order not in (0, 1): raise ValueError("order 0 (local constant) or 1 (local linear)")
        self.key, self.kernel, self.order, self.interpolation = key, kernel, int(order), interpolation
        _kernel(kernel)
        self.points = default_points(key, 64 if points is None else int(points)) if points is None or np.isscalar(points) else np.asarray(points, dtype=np.float64).ravel()
        if not 1 <= self.points.size <= MAX_POINTS: raise ValueError(f"1 … {MAX_POINTS} points")
        if bandwidths is None:
            spacing = float(np.diff(self.points).max()) if self.points.size > 1 else 0.0
            bandwidths = max(3.0 * silverman_bandwidth(key), 1.5 * spacing)
        self.points, self.bandwidths = _grid(self.points, bandwidths)

    def getMoments(self, dependents) -> np.ndarray:
        return kernel_moments(self.key, self.points, self.bandwidths, dependents, self.kernel, self.order)

    def getFittedValues(self, dependents) -> np.ndarray:
        """The estimate at the points: [Q] for one dependent, [M, Q] for a sequence of M (one launch per four of them)."""
        one = not isinstance(dependents, (list, tuple))
        ys = [dependents] if one else list(dependents)
        rows = []
        for m0 in range(0, len(ys), MAX_Y):
            part = ys[m0:m0 + MAX_Y]
            rows.append(kernel_local_fit(self.getMoments(part), self.order, len(part), self.points)[0])
        values = np.concatenate(rows, axis=0)
        return values[0] if one else values

    def _table(self, fitted) -> TabulatedFunction:
        keep = np.concatenate([[True], np.diff(self.points) > 0.0])               # a table's knots are strictly increasing
        return TabulatedFunction(self.points[keep], np.asarray(fitted)[keep], self.interpolation, "constant")

    def _apply(self, f: TabulatedFunction):
        try: return self.key.apply(f)
        except (AttributeError, NotImplementedError, TypeError):
            return type(self.key)(self.key.getFiltrationTime(), table_apply_host(_host_values(self.key), [f])[0])

    def getConditionalExpectation(self, dependents):
        """Per path the interpolated estimate at its key: key.apply(TabulatedFunction(points, fitted values))."""
        fitted = self.getFittedValues(dependents)
        if fitted.ndim == 1: return self._apply(self._table(fitted))
        return [self._apply(self._table(row)) for row in fitted]
