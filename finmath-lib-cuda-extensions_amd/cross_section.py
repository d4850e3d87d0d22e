"""Order statistics ACROSS vectors, per path (include/fmhip.h: fmhip_cross_order_statistics, fmhip_cross_select): the
largest, second largest, r-th largest of K assets on every path and WHICH asset it is, without the vectors leaving the device — best-of,
worst-of, rainbow and mountain-range payoffs, the r-th default of a basket, and the regression basis of ordered prices that the Bermudan
max-call wants (montecarlo.bermudan_max_call_mc(ordered_states=True), montecarlo.best_of_call_mc).

For path p the K pairs (key of vs[i][p], i) are sorted ascending by the 32-bit key of the other order statistics — the order of
java.util.Arrays.sort(float[]): −0.0 before +0.0, every NaN equal and last — ties by slot i (a stable sort).  A value output is one of the
path's K values bit for bit (a NaN comes back as the quiet NaN 0x7fc00000); an index output is the slot as a float.  select_across carries
a payload behind an index: out[p] = vs[index[p]][p], the quiet NaN where index[p] is no integer in [0, K).  The device's bits are those of
fmhip_cross_order_statistics_host and fmhip_cross_select_host (host/cross_order.hpp, the definition).

FMHIP_DEVICE_CROSS_ORDER=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition runs on one core,
and the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

VALUES, INDICES = 1, 2                                               # FMHIP_CROSS_VALUES, FMHIP_CROSS_INDICES
MAX_VECTORS, MAX_RANKS = 32, 32                                      # FM_CROSS_MAX_VECTORS, FM_CROSS_MAX_RANKS (host/cross_order.hpp)


def device_cross_order() -> bool:
    """FMHIP_DEVICE_CROSS_ORDER=0: the calls download their vectors, run the definition on the host and upload the results (the A/B switch and
    the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_CROSS_ORDER", "1") != "0"


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def _mask(values, indices, what):
    mask = (VALUES if values else 0) | (INDICES if indices else 0)
    if not mask: raise ValueError(f"{what}: neither values nor indices")
    return mask


def _ranks(ranks, k, what):
    ranks = [int(r) for r in ranks]
    if not ranks: raise ValueError(f"{what}: no rank")
    for r in ranks:
        if not 0 <= r < k: raise ValueError(f"{what}: rank {r} of {k} vectors")
    return ranks


def cross_order_statistics_host(arrays, ranks, values=True, indices=False) -> list:
    """The DEFINITION (fmhip_cross_order_statistics_host): [one float32 array per rank of values] + [one per rank of indices]; needs no device.
    Any number of selectors: they are taken 32 at a time."""
    arrays = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in arrays]
    mask = _mask(values, indices, "cross_order_statistics_host")
    ranks = [int(r) for r in ranks]
    n = arrays[0].size if arrays else 0
    kinds = (1 if values else 0) + (1 if indices else 0)
    got = [None] * (kinds * len(ranks))
    for at in range(0, max(len(ranks), 1), MAX_RANKS):
        part = ranks[at:at + MAX_RANKS]
        out = [np.empty(max(n, 1), dtype=np.float32) for _ in range(kinds * len(part))]
        N.check(N.lib().fmhip_cross_order_statistics_host(_pointers(arrays), len(arrays), n, (C.c_int32 * max(len(part), 1))(*part), len(part), mask, _pointers(out)))
        for kind in range(kinds):
            for j in range(len(part)): got[kind * len(ranks) + at + j] = out[kind * len(part) + j][:n]
    return got


def cross_select_host(index, arrays) -> np.ndarray:
    """The DEFINITION (fmhip_cross_select_host): out[p] = arrays[index[p]][p] bit for bit, the quiet NaN where index[p] is no integer in [0, K)."""
    index = np.ascontiguousarray(index, dtype=np.float32).ravel()
    arrays = [np.ascontiguousarray(a, dtype=np.float32).ravel() for a in arrays]
    out = np.empty(max(index.size, 1), dtype=np.float32)
    N.check(N.lib().fmhip_cross_select_host(index.ctypes.data_as(C.c_void_p), _pointers(arrays), len(arrays), index.size, out.ctypes.data_as(C.c_void_p)))
    return out[:index.size]


def _operands(vs, what, most=MAX_VECTORS):
    """(time, [DeviceVector], n, all deterministic?): deterministic variables among stochastic ones become filled vectors of their size."""
    vs = list(vs)
    if not 1 <= len(vs) <= most: raise ValueError(f"{what} of {len(vs)} vectors: 1 … {most}")
    args = []
    for v in vs:
        if isinstance(v, RandomVariableHip): args.append((v.time, v.realizations, v.value))
        elif isinstance(v, DeviceVector): args.append((-math.inf, v, math.nan))
        else: raise TypeError(f"{what}: of RandomVariableHip or DeviceVector, not {type(v).__name__}")
    time = max(t for t, _, _ in args)
    sizes = {dv.n for _, dv, _ in args if dv is not None}
    if len(sizes) > 1: raise ValueError(f"{what}: vectors of different sizes {sorted(sizes)}")
    if not sizes: return time, None, 1, [float(np.float32(value)) for _, _, value in args]
    n = next(iter(sizes))
    return time, [dv if dv is not None else DeviceVector.filled(n, value) for _, dv, value in args], n, None


def order_across(vs, ranks, values=True, indices=False) -> list:
    """[the ranks[j]-th smallest of vs[0][p] … vs[K−1][p] for j] (values), then [the slot it came from, as a float, for j] (indices), as
    RandomVariableHip: K = len(vs) <= 32 variables of one size, rank 0 the smallest and K − 1 the largest, ties by slot.  One launch per 32
    selectors.  Deterministic variables alone give deterministic results."""
    mask = _mask(values, indices, "order_across")
    vs = list(vs)
    time, dvs, n, constants = _operands(vs, "order_across")
    ranks = _ranks(ranks, len(vs) if dvs is None else len(dvs), "order_across")
    kinds = (1 if values else 0) + (1 if indices else 0)
    if dvs is None:
        got = cross_order_statistics_host([np.float32([c]) for c in constants], ranks, values, indices)
        return [RandomVariableHip(time, float(g[0])) for g in got]
    if not device_cross_order():
        return [RandomVariableHip(time, DeviceVector.from_host(g)) for g in cross_order_statistics_host([dv.to_float32() for dv in dvs], ranks, values, indices)]
    handles = (C.c_int64 * len(dvs))(*[dv.handle for dv in dvs])
    made = [None] * (kinds * len(ranks))
    for at in range(0, len(ranks), MAX_RANKS):
        part = ranks[at:at + MAX_RANKS]
        out = (C.c_int64 * (kinds * len(part)))()
        N.check(N.lib().fmhip_cross_order_statistics(handles, len(dvs), (C.c_int32 * len(part))(*part), len(part), mask, out))
        for kind in range(kinds):
            for j in range(len(part)): made[kind * len(ranks) + at + j] = DeviceVector(int(out[kind * len(part) + j]), n)
    return [RandomVariableHip(time, dv) for dv in made]


def sort_across(vs, descending=False) -> list:
    """The K variables sorted per path: [smallest, …, largest], or with descending [largest, …, smallest]."""
    vs = list(vs)
    k = len(vs)
    return order_across(vs, range(k - 1, -1, -1) if descending else range(k))


def max_across(vs) -> RandomVariableHip:
    """The largest of the K values of every path in the order of Arrays.sort: a NaN, if the path holds one."""
    vs = list(vs)
    return order_across(vs, [len(vs) - 1])[0]


def min_across(vs) -> RandomVariableHip:
    """The smallest of the K values of every path (−0.0 before +0.0)."""
    vs = list(vs)
    return order_across(vs, [0])[0]


def median_across(vs) -> RandomVariableHip:
    """The lower median: rank (K − 1) // 2 of the K values of every path."""
    vs = list(vs)
    return order_across(vs, [(len(vs) - 1) // 2])[0]


def argmax_across(vs) -> RandomVariableHip:
    """The slot of the largest value of every path, as a float; among equal values the LAST slot (the stable sort's)."""
    vs = list(vs)
    return order_across(vs, [len(vs) - 1], values=False, indices=True)[0]


def argmin_across(vs) -> RandomVariableHip:
    """The slot of the smallest value of every path, as a float; among equal values the first slot."""
    vs = list(vs)
    return order_across(vs, [0], values=False, indices=True)[0]


def select_across(index, vs) -> RandomVariableHip:
    """out[p] = vs[index[p]][p] bit for bit; the quiet NaN where index[p] is no integer in [0, K): the payload behind an index output."""
    vs = list(vs)
    if not 1 <= len(vs) <= MAX_VECTORS: raise ValueError(f"select_across among {len(vs)} vectors: 1 … {MAX_VECTORS}")
    time, dvs, n, constants = _operands([index] + vs, "select_across", MAX_VECTORS + 1)
    if dvs is None:
        return RandomVariableHip(time, float(cross_select_host(np.float32([constants[0]]), [np.float32([c]) for c in constants[1:]])[0]))
    if not device_cross_order():
        return RandomVariableHip(time, DeviceVector.from_host(cross_select_host(dvs[0].to_float32(), [dv.to_float32() for dv in dvs[1:]])))
    handles = (C.c_int64 * (len(dvs) - 1))(*[dv.handle for dv in dvs[1:]])
    h = C.c_int64(0)
    N.check(N.lib().fmhip_cross_select(dvs[0].handle, handles, len(dvs) - 1, C.byref(h)))
    return RandomVariableHip(time, DeviceVector(h.value, n))
