"""Prefix sums on the device (include/fmhip.h: fmhip_prefix_sums, fmhip_prefix_sums_at, fmhip_prefix_search): the running
sum along a sample without the vector leaving the device — and what a WEIGHTED sample (importance sampling, likelihood-ratio weights,
weighted Monte-Carlo) needs behind the sort of §4.16: a weighted quantile, a weighted expected shortfall, the whole expected-shortfall curve
of a loss vector, the running average of an estimator against the number of paths.

P[r] is the fp64 sum of v[0..r] in ONE tree, a function of the size and of r alone (csrc/prefix_host.hpp): the device's bits are those of
fmhip_prefix_sums_host, and for input without negative elements or NaNs P is non-decreasing — a cumulative weight is a CDF.

FMHIP_DEVICE_PREFIX=0, read per call: the A/B switch and the fallback — the vector is downloaded, fmhip_prefix_sums_host (the definition)
runs, and what is a vector is uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector
from .sorting import _vector, read_elements, sort_by_key

MAX_QUERIES = 4096
SUM, MEAN = 0, 1


def device_prefix() -> bool:
    """FMHIP_DEVICE_PREFIX=0: prefix sums download the vector, run the definition on the host and upload what is a vector (the A/B switch
    and the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_PREFIX", "1") != "0"


def prefix_sums_host(a) -> np.ndarray:
    """The DEFINITION (fmhip_prefix_sums_host): P[r] in float64 for a host array; needs no device."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    out = np.empty(a.size, dtype=np.float64)
    N.check(N.lib().fmhip_prefix_sums_host(a.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def _queries(q, dtype, what):
    q = np.ascontiguousarray(q, dtype=dtype).ravel()
    if not 1 <= q.size <= MAX_QUERIES: raise ValueError(f"{what}: {q.size} queries (1 … {MAX_QUERIES} in one call)")
    return q


def cumulative_sums(v, mean: bool = False, with_total: bool = False):
    """out[r] = (float32)P[r] as a new DeviceVector, or with mean=True (float32)(P[r] / (r + 1)): the running average.  with_total: also P[n-1]."""
    v = _vector(v)
    if not device_prefix():
        p = prefix_sums_host(v.to_float32())
        out = DeviceVector.from_host((p / np.arange(1, v.n + 1, dtype=np.float64) if mean else p).astype(np.float32))
        return (out, float(p[-1])) if with_total else out
    h = C.c_int64(0)
    total = C.c_double(0.0)
    N.check(N.lib().fmhip_prefix_sums(v.handle, MEAN if mean else SUM, C.byref(h), C.byref(total)))
    out = DeviceVector(h.value, v.n)
    return (out, total.value) if with_total else out


def running_average(v) -> DeviceVector:
    """out[r] = the mean of v[0..r]: an estimator against the number of paths."""
    return cumulative_sums(v, mean=True)


def prefix_sums_at(v, positions) -> np.ndarray:
    """(float64) P[positions]: up to 4096 prefix sums without writing a vector; any order, repeats allowed."""
    v = _vector(v)
    p = _queries(positions, np.int64, "prefix_sums_at")
    if ((p < 0) | (p >= v.n)).any(): raise ValueError(f"prefix_sums_at: a position outside [0, {v.n})")
    if not device_prefix():
        return prefix_sums_host(v.to_float32())[p]
    out = np.empty(p.size, dtype=np.float64)
    N.check(N.lib().fmhip_prefix_sums_at(v.handle, p.ctypes.data_as(C.POINTER(C.c_int64)), p.size, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def prefix_search(v, thresholds, relative: bool = False):
    """(positions, sums, total): positions[j] = the smallest r with P[r] >= t_j (int64), sums[j] = that P[r]; n and P[n-1] where no prefix
    reaches t_j.  t_j = thresholds[j], or thresholds[j]·P[n-1] (one fp64 product) with relative=True.  A NaN never qualifies."""
    v = _vector(v)
    t = _queries(thresholds, np.float64, "prefix_search")
    if not device_prefix():
        p = prefix_sums_host(v.to_float32())
        total = p[-1]
        tt = t * total if relative else t
        pos = np.empty(t.size, dtype=np.int64)
        for j, x in enumerate(tt):
            hit = p >= x                                             # (a NaN on either side: False)
            pos[j] = int(np.argmax(hit)) if hit.any() else v.n
        return pos, np.where(pos < v.n, p[np.minimum(pos, v.n - 1)], total), float(total)
    pos = np.empty(t.size, dtype=np.int64)
    sums = np.empty(t.size, dtype=np.float64)
    total = C.c_double(0.0)
    N.check(N.lib().fmhip_prefix_search(v.handle, t.ctypes.data_as(C.POINTER(C.c_double)), t.size, 1 if relative else 0,
                                        pos.ctypes.data_as(C.POINTER(C.c_int64)), sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(total)))
    return pos, sums, total.value


def weighted_quantiles(x, w, levels) -> np.ndarray:
    """The inverted weighted CDF at every level: the element of x at the smallest position of the ascending sample whose cumulative weight
    reaches level·W, W the sum of the weights; ties of x in path order.  ONE sort_by_key(x, [w]), one relative search, one read_elements.
    NaN where no position qualifies (a NaN level, a level above 1)."""
    x, w = _vector(x), _vector(w)
    sx, (sw,) = sort_by_key(x, [w])
    pos, _, _ = prefix_search(sw, levels, relative=True)
    found = pos < x.n
    out = np.full(pos.size, np.nan, dtype=np.float64)
    if found.any(): out[found] = read_elements(sx, pos[found])
    return out


def weighted_expected_shortfall(x, w, level: float) -> float:
    """Σ w·x / Σ w over the positions of the ascending sample up to the weighted quantile's: the weighted mean of the tail below the level.
    Two prefix_sums_at calls behind the sort and the search: one on the sorted weights, one on their fp32 product with the sorted values."""
    x, w = _vector(x), _vector(w)
    sx, (sw,) = sort_by_key(x, [w])
    pos, _, _ = prefix_search(sw, [level], relative=True)
    if pos[0] >= x.n: return float("nan")
    return float(prefix_sums_at(sw.v2s0("MULT", sx), pos)[0] / prefix_sums_at(sw, pos)[0])


def expected_shortfall_curve(x) -> DeviceVector:
    """out[r] = the mean of the r + 1 smallest elements of x: the whole expected-shortfall curve, one sort and one prefix pass."""
    sx, _ = sort_by_key(_vector(x))
    return cumulative_sums(sx, mean=True)
