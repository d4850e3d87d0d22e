"""Reduce by key on the device (include/fmhip.h: fmhip_group_sums and its _host twin): out[k] = Σ { v[j] : index[j] == k } —
reduce_by_key, index_add, bincount(weights=) — for an index vector that another pass left on the device: the ancestors of a resample
(offspring_counts), the slot of argmax_across, a bin number, a Poisson count (conditional_expectation_by_state; the driver
montecarlo.merton_call_by_jump_count_mc), inner paths of unequal number, histograms of any number of bins.

The definition is csrc/group_host.hpp, one header for the host and the device: element j belongs to group k where index[j] is the integer k
in [0, m - 1] (-0.0 counts as 0) and to NO group anywhere else (NaN, ±inf, a fraction, negative, >= m — never an error: such elements are
counted as `ungrouped`); the members of a group are summed in ascending path order in fp64, as run-prefixes of the prefix sums' tree over
the elements ordered by (group, path).  The outputs — count, sum, mean, variance per group, vectors of m elements — are rounded to float32
once; an empty group has count 0, sum +0.0, mean and variance NaN.  The device's bits are the host twin's for every input.

FMHIP_DEVICE_GROUP=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition runs on one core, and
the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip
from .selection import _argument, _columns, _floats, gather

MAX_VALUES = 4
MAX_GROUPS = 1 << 24
WHAT = {"sum": 1, "mean": 2, "variance": 4}          # FMHIP_BLOCK_SUM, FMHIP_BLOCK_MEAN, FMHIP_BLOCK_VARIANCE


def device_group() -> bool:
    """FMHIP_DEVICE_GROUP=0: the group passes download their vectors, run the definition on the host and upload the results (the A/B
    switch and the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_GROUP", "1") != "0"


def _mask(what):
    """(mask, slots): the bits of `what` and, per entry of `what`, its place among the mask's bits in ascending order."""
    what = (what,) if isinstance(what, str) else tuple(what)
    for w in what:
        if w not in WHAT: raise ValueError(f"group moments: {w!r} is none of 'sum', 'mean', 'variance'")
    if len(set(what)) != len(what): raise ValueError("group moments: an output named twice")
    mask = sum(WHAT[w] for w in what)
    order = [w for w in ("sum", "mean", "variance") if w in what]
    return mask, [order.index(w) for w in what]


def _check(m, k, mask, anything_else):
    if not isinstance(m, (int, np.integer)) or not 1 <= m <= MAX_GROUPS: raise ValueError(f"group moments: m = {m!r}: an integer 1 … 2^24")
    if not 0 <= k <= MAX_VALUES: raise ValueError(f"group moments of {k} value vectors: 0 … {MAX_VALUES} in one call")
    if k > 0 and mask == 0: raise ValueError("group moments: value vectors and no output named")
    if k == 0 and not anything_else: raise ValueError("group moments: nothing asked for")


# ---------------------------------------------------------------- the definition over numpy arrays
def group_sums_host(index, values, m, what=("sum",)):
    """The DEFINITION (fmhip_group_sums_host); needs no device.  Returns (outs, counts, ungrouped): outs[i][j] a float32 array of m
    elements for value vector i and entry j of `what`, counts a float32 array of m elements, ungrouped an int."""
    index = _floats(index)
    values = [_floats(v) for v in values]
    mask, slots = _mask(what) if values else (0, [])
    _check(m, len(values), mask, True)
    for v in values:
        if v.size != index.size: raise ValueError("group sums: a value vector whose size is not the index's")
    per = len(slots)
    outs = [np.empty(m, dtype=np.float32) for _ in range(len(values) * per)]
    counts = np.empty(m, dtype=np.float32)
    ungrouped = C.c_int64(-1)
    N.check(N.lib().fmhip_group_sums_host(index.ctypes.data_as(C.c_void_p), index.size, int(m), _columns(values) if values else None, len(values), mask,
                                          counts.ctypes.data_as(C.c_void_p), _columns(outs) if outs else None, C.byref(ungrouped)))
    return [[outs[i * per + s] for s in slots] for i in range(len(values))], counts, ungrouped.value


# ---------------------------------------------------------------- the mirror
def group_moments(index, values, m, what=("sum",), counts=False):
    """Per group k = 0 … m - 1 of `index` the outputs named in `what` ('sum', 'mean', 'variance') of up to 4 value vectors of the index's
    size.  Returns (outs, counts, ungrouped): outs[i][j] a RandomVariableHip of m elements for value vector i and entry j of `what`; counts
    the count per group as a RandomVariableHip (None unless counts=True); ungrouped the number of elements that belong to no group.
    Filtration time: the later of the index's and the value vector's; the counts have the index's."""
    i_time, ix = _argument(index, "group moments")
    args = [_argument(v, "group moments") for v in values]
    mask, slots = _mask(what) if args else (0, [])
    _check(m, len(args), mask, True)
    for _, v in args:
        if v.n != ix.n: raise ValueError("group moments: a value vector whose size is not the index's")
    per = len(slots)
    m = int(m)
    if not device_group():
        outs, cnt, ungrouped = group_sums_host(ix.to_float32(), [v.to_float32() for _, v in args], m, what if args else ())
        made = [[RandomVariableHip(max(i_time, t), DeviceVector.from_host(o)) for o in row] for (t, _), row in zip(args, outs)]
        return made, (RandomVariableHip(i_time, DeviceVector.from_host(cnt)) if counts else None), ungrouped
    hv = (C.c_int64 * max(len(args), 1))(*[v.handle for _, v in args])
    out = (C.c_int64 * max(len(args) * per, 1))()
    out_counts = C.c_int64(0)
    ungrouped = C.c_int64(-1)
    N.check(N.lib().fmhip_group_sums(ix.handle, m, hv if args else None, len(args), mask, C.byref(out_counts) if counts else None, out if args else None, C.byref(ungrouped)))
    made = [[RandomVariableHip(max(i_time, t), DeviceVector(int(out[i * per + s]), m)) for s in slots] for i, (t, _) in enumerate(args)]
    return made, (RandomVariableHip(i_time, DeviceVector(out_counts.value, m)) if counts else None), ungrouped.value


def group_sums(index, values, m):
    """The sum per group of every value vector: a list of RandomVariableHip of m elements."""
    return [row[0] for row in group_moments(index, values, m, what=("sum",))[0]]


def group_means(index, values, m):
    """The mean per group of every value vector (NaN for an empty group): a list of RandomVariableHip of m elements."""
    return [row[0] for row in group_moments(index, values, m, what=("mean",))[0]]


def group_counts(index, m):
    """(counts, ungrouped): the number of elements per group as a RandomVariableHip of m elements (float32: exact up to 2^24 per group)
    and the number of elements that belong to no group."""
    _, counts, ungrouped = group_moments(index, [], m, what=(), counts=True)
    return counts, ungrouped


def conditional_expectation_by_state(index, y, m):
    """E[y | state] back on every path: the mean of y over the paths with the same integer state index[j] in [0, m - 1] — gather(index,
    [group_means]).  A path whose state is no integer in that range receives the quiet NaN."""
    (mean,) = group_means(index, [y], m)
    return gather(index, [mean])[0]


def offspring_counts(ancestors, n):
    """How often each of n paths was drawn by a resample: the counts per group of its ancestors, a RandomVariableHip of n elements."""
    return group_counts(ancestors, n)[0]
