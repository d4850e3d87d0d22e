"""Sort on the device (include/fmhip.h: fmhip_sort_by_key, fmhip_argsort, fmhip_rank_scores, fmhip_vec_read_elements): the
whole ordered sample, the permutation and the ranks per path without the vector leaving the device — an expected-shortfall curve, a PFE
profile at a hundred levels, companions reordered by a state, empirical-CDF scores, Spearman's rank correlation.

The order is the order statistics' (§4.7): ascending in the 32-bit key — java.util.Arrays.sort(float[])'s order, −0.0 before +0.0, every NaN
last — and STABLE: ties keep ascending path order.  Ranks are ordinal (ties by path index); midranks and descending order are not offered.

FMHIP_DEVICE_SORT=0, read per call: the A/B switch and the fallback — the key is downloaded, numpy's stable argsort runs on the same keys,
and the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip, quantile_index

MAX_VALUES = 8


def device_sort() -> bool:
    """FMHIP_DEVICE_SORT=0: sorts download the key, order it on the host (numpy's stable argsort of the keys) and upload the results (the
    A/B switch and the fallback); anything else: sorted on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_SORT", "1") != "0"


def sort_keys(a) -> np.ndarray:
    """The 32-bit keys whose unsigned order is the sort's (the key of the order statistics): u = bits(x); (u >> 31) ? ~u : u | 0x80000000,
    every NaN 0xFFFFFFFF."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    k = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(a), np.uint32(0xFFFFFFFF), k).astype(np.uint32)


def _vector(v) -> DeviceVector:
    if isinstance(v, RandomVariableHip):
        if v.isDeterministic(): raise ValueError("a deterministic random variable has no vector to sort")
        v = v.realizations
    if not isinstance(v, DeviceVector): raise TypeError("a RandomVariableHip or a DeviceVector is sorted, not " + type(v).__name__)
    return v


def _host_permutation(key: DeviceVector) -> np.ndarray:
    return np.argsort(sort_keys(key.to_float32()), kind="stable").astype(np.int64)


def argsort(key) -> np.ndarray:
    """permutation[r] = the path at position r of the ascending sample (int64, on the host); equal keys in ascending path order."""
    key = _vector(key)
    if not device_sort():
        return _host_permutation(key)
    out = np.empty(key.n, dtype=np.int64)
    N.check(N.lib().fmhip_argsort(key.handle, out.ctypes.data_as(C.POINTER(C.c_int64))))
    return out


def sort_by_key(key, values=()):
    """(sorted key, [sorted values…]) as new DeviceVectors: out[r] = in[permutation[r]] for the key and up to 8 companion vectors of its
    size, copied bit for bit (a NaN keeps its payload, a zero its sign).  One sort, one gather; the inputs are unchanged."""
    key = _vector(key)
    values = [_vector(v) for v in values]
    if len(values) > MAX_VALUES: raise ValueError(f"sort_by_key with {len(values)} companion vectors: at most {MAX_VALUES} in one call")
    for v in values:
        if v.n != key.n: raise ValueError("sort_by_key over vectors of different size")
    if not device_sort():
        perm = _host_permutation(key)
        up = lambda v: DeviceVector.from_host(v.to_float32()[perm])
        return up(key), [up(v) for v in values]
    hv = (C.c_int64 * max(len(values), 1))(*[v.handle for v in values])
    out_key = C.c_int64(0)
    out_values = (C.c_int64 * max(len(values), 1))()
    N.check(N.lib().fmhip_sort_by_key(key.handle, hv if values else None, len(values), C.byref(out_key), out_values if values else None))
    return DeviceVector(out_key.value, key.n), [DeviceVector(out_values[i], key.n) for i in range(len(values))]


def rank_scores(key) -> DeviceVector:
    """out[p] = (float32)((rank(p) + 0.5) / n) as a new DeviceVector: the empirical-CDF score of every path, ordinal ranks (ties by path
    index), strictly inside (0, 1)."""
    key = _vector(key)
    if not device_sort():
        perm = _host_permutation(key)
        inverse = np.empty(key.n, dtype=np.int64)
        inverse[perm] = np.arange(key.n, dtype=np.int64)
        return DeviceVector.from_host(((inverse + 0.5) / key.n).astype(np.float32))
    out = C.c_int64(0)
    N.check(N.lib().fmhip_rank_scores(key.handle, C.byref(out)))
    return DeviceVector(out.value, key.n)


def read_elements(v, positions) -> np.ndarray:
    """(float64) v[positions]: a few elements of a vector without reading the vector (fmhip_vec_read_elements); repeats allowed."""
    v = _vector(v)
    p = np.ascontiguousarray(positions, dtype=np.int64).ravel()
    out = np.empty(p.size, dtype=np.float64)
    N.check(N.lib().fmhip_vec_read_elements(v.handle, p.ctypes.data_as(C.POINTER(C.c_int64)), p.size, out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def sorted_quantiles(v, quantiles) -> np.ndarray:
    """getQuantile(q) for every q of a list from ONE sort and ONE read of the selected elements: the element at quantile_index(n, q) of the
    ascending sample, level by level what getQuantile returns."""
    v = _vector(v)
    ranks = [quantile_index(v.n, float(q)) for q in np.asarray(quantiles, dtype=np.float64).ravel()]
    if not ranks: return np.empty(0, dtype=np.float64)
    if not device_sort():
        a = v.to_float32()
        return a[_host_permutation(v)][ranks].astype(np.float64)
    ordered, _ = sort_by_key(v)
    return read_elements(ordered, ranks)


def spearman_matrix(vectors) -> np.ndarray:
    """Spearman's rank correlation of up to 63 vectors: the covariance matrix of their rank scores (one sort per vector, ONE cross-moments
    pass for all of them), normalised to correlations; exactly 1 on the diagonal.  Ordinal ranks: ties are broken by path index."""
    from .regression import covariance_matrix
    scores = [rank_scores(v) for v in vectors]
    cov = covariance_matrix(scores)
    sd = np.sqrt(np.diag(cov))
    corr = cov / np.outer(sd, sd)
    np.fill_diagonal(corr, 1.0)
    return corr
