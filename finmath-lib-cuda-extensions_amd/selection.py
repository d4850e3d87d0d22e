"""Selection on the device (include/fmhip.h: fmhip_compress, fmhip_expand, fmhip_gather and their _host twins): keep the
paths on which a condition holds — copy_if —, put them back, and read by an index.  Longstaff–Schwartz on the in-the-money paths
(montecarlo.bermudan_option_mc(in_the_money_only=True)), the quantile or tail mean of a loss given a barrier hit (getQuantile of the
compressed vector), rare events whose downstream launches should run on 1 % of the paths, one index list carried to any number of vectors.

The definition is csrc/select_host.hpp, one header for the host and the device: an element is SELECTED where mask >= 0 in float32, the
trigger of choose (a NaN is not, -0.0 is, +inf is); compress keeps the selected paths in path order, bit for bit, as vectors of exactly
`count` elements; expand is its inverse with a fill on the other paths; gather reads values[index[j]] and gives the quiet NaN where the
index is no integer in [0, n - 1].  Counts are integers: the device's bits are the host twins' for every input.

FMHIP_DEVICE_SELECT=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition runs on one core, and
the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

MAX_VALUES = 8
MAX_POSITION_N = 1 << 24


def device_select() -> bool:
    """FMHIP_DEVICE_SELECT=0: compress, expand and gather download their vectors, run the definition on the host and upload the results
    (the A/B switch and the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_SELECT", "1") != "0"


def _argument(v, what):
    """(time, DeviceVector): a RandomVariableHip keeps its filtration time; a bare DeviceVector has none (-inf)."""
    if isinstance(v, RandomVariableHip):
        if v.isDeterministic(): raise ValueError(f"{what}: a deterministic random variable has no vector")
        return v.time, v.realizations
    if isinstance(v, DeviceVector):
        return -math.inf, v
    raise TypeError(f"{what}: of a RandomVariableHip or a DeviceVector, not {type(v).__name__}")


def _floats(a):
    return np.ascontiguousarray(a, dtype=np.float32).ravel()


def _columns(arrays):
    return (C.c_void_p * max(len(arrays), 1))(*[a.ctypes.data for a in arrays])


def _check_count(what, k, least):
    if not least <= k <= MAX_VALUES: raise ValueError(f"{what} of {k} value vectors: {least} … {MAX_VALUES} in one call")


# ---------------------------------------------------------------- the definitions over numpy arrays
def compress_host(mask, values, positions=False):
    """The DEFINITION (fmhip_compress_host); needs no device.  Returns (outs, count), or (outs, positions, count) with positions=True:
    one float32 array of `count` elements per value vector, the positions as int64."""
    mask = _floats(mask)
    values = [_floats(v) for v in values]
    n = mask.size
    for v in values:
        if v.size != n: raise ValueError("compress: a value vector whose size is not the mask's")
    outs = [np.empty(max(n, 1), dtype=np.float32) for _ in values]
    pos = np.empty(max(n, 1), dtype=np.int64) if positions else None
    count = C.c_int64(-1)
    N.check(N.lib().fmhip_compress_host(mask.ctypes.data_as(C.c_void_p), n, _columns(values) if values else None, len(values), _columns(outs) if values else None,
                                        None if pos is None else pos.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(count)))
    outs = [o[:count.value].copy() for o in outs]
    return (outs, pos[:count.value].copy(), count.value) if positions else (outs, count.value)


def expand_host(mask, values, fill=0.0):
    """The DEFINITION (fmhip_expand_host): one float32 array of the mask's size per value vector; values whose size is not the
    mask's count are FMHIP_ERR_SIZE_MISMATCH (FmhipError)."""
    mask = _floats(mask)
    values = [_floats(v) for v in values]
    k = values[0].size if values else 0
    for v in values:
        if v.size != k: raise ValueError("expand: value vectors of different size")
    held = [v if v.size else np.zeros(1, dtype=np.float32) for v in values]          # (an empty array has no address worth passing)
    outs = [np.empty(max(mask.size, 1), dtype=np.float32) for _ in values]
    N.check(N.lib().fmhip_expand_host(mask.ctypes.data_as(C.c_void_p), mask.size, _columns(held) if values else None, len(values), k, float(fill),
                                      _columns(outs) if values else None))
    return [o[:mask.size] for o in outs]


def gather_host(index, values, n=None):
    """The DEFINITION (fmhip_gather_host): out[i][j] = values[i][index[j]], the quiet NaN where index[j] is no integer in [0, n - 1].  n
    defaults to the size of the values; a larger n may be stated where the index is known not to reach beyond the arrays given."""
    index = _floats(index)
    values = [_floats(v) for v in values]
    size = values[0].size if values else 0
    for v in values:
        if v.size != size: raise ValueError("gather: value vectors of different size")
    if n is None: n = size
    outs = [np.empty(max(index.size, 1), dtype=np.float32) for _ in values]
    N.check(N.lib().fmhip_gather_host(index.ctypes.data_as(C.c_void_p), index.size, _columns(values) if values else None, len(values), int(n),
                                      _columns(outs) if values else None))
    return [o[:index.size] for o in outs]


# ---------------------------------------------------------------- the mirror
def compress(mask, values, positions=False):
    """The paths of `values` (up to 8 vectors of the mask's size) on which mask >= 0, in path order, bit for bit.  Returns
    (list_of_vectors, count): one RandomVariableHip of `count` paths per value vector and, with positions=True, the positions (float32,
    exact: offered up to 2^24 paths) as the last entry.  count == 0 gives None in place of every vector: an empty vector is not a vector.
    Filtration time: an output has the later of the mask's time and its value vector's; the positions have the mask's."""
    m_time, m = _argument(mask, "compress")
    args = [_argument(v, "compress") for v in values]
    _check_count("compress", len(args), 0)
    for _, v in args:
        if v.n != m.n: raise ValueError("compress: a value vector whose size is not the mask's")
    if positions and m.n > MAX_POSITION_N: raise ValueError("compress: the positions are offered up to 2^24 elements, where the float is exact")
    times = [max(m_time, t) for t, _ in args] + ([m_time] if positions else [])
    if not device_select():
        got = compress_host(m.to_float32(), [v.to_float32() for _, v in args], positions)
        outs, count = got[0], got[-1]
        if positions: outs = outs + [got[1].astype(np.float32)]
        if count == 0: return [None] * len(times), 0
        return [RandomVariableHip(t, DeviceVector.from_host(o)) for t, o in zip(times, outs)], count
    hv = (C.c_int64 * max(len(args), 1))(*[v.handle for _, v in args])
    out_values = (C.c_int64 * max(len(args), 1))()
    out_positions = C.c_int64(0)
    count = C.c_int64(0)
    N.check(N.lib().fmhip_compress(m.handle, hv if args else None, len(args), out_values if args else None, C.byref(out_positions) if positions else None, C.byref(count)))
    if count.value == 0: return [None] * len(times), 0
    handles = [int(out_values[i]) for i in range(len(args))] + ([out_positions.value] if positions else [])
    return [RandomVariableHip(t, DeviceVector(h, count.value)) for t, h in zip(times, handles)], count.value


def count_selected(mask) -> int:
    """The number of paths with mask >= 0: the first phase of a compress alone, one integer leaves the device."""
    return compress(mask, [])[1]


def expand(mask, values, fill=0.0):
    """The inverse of compress: one RandomVariableHip of the mask's size per entry of `values`, values[i][q(r)] on the selected paths and
    float32(fill) — which may be ±inf or NaN — on the others.  Every vector has exactly count_selected(mask) elements (FmhipError with
    FMHIP_ERR_SIZE_MISMATCH otherwise, found after the count).  A None entry — what compress gives at count == 0 — gives the
    constant fill.  Filtration time: the later of the mask's and the value vector's."""
    m_time, m = _argument(mask, "expand")
    entries = list(values)
    args = [_argument(v, "expand") for v in entries if v is not None]
    if args: _check_count("expand", len(args), 1)
    made = []
    if args:
        times = [max(m_time, t) for t, _ in args]
        if not device_select():
            outs = expand_host(m.to_float32(), [v.to_float32() for _, v in args], fill)
            made = [RandomVariableHip(t, DeviceVector.from_host(o)) for t, o in zip(times, outs)]
        else:
            hv = (C.c_int64 * len(args))(*[v.handle for _, v in args])
            out = (C.c_int64 * len(args))()
            N.check(N.lib().fmhip_expand(m.handle, hv, len(args), float(fill), out))
            made = [RandomVariableHip(t, DeviceVector(int(out[i]), m.n)) for i, t in enumerate(times)]
    made = iter(made)
    return [RandomVariableHip(m_time, DeviceVector.from_host(np.full(m.n, fill, dtype=np.float32))) if v is None else next(made) for v in entries]


def gather(index, values):
    """out[i][j] = values[i][index[j]] bit for bit, as RandomVariableHip of the index's size; the quiet NaN where index[j] is no integer in
    [0, n - 1] (-0.0 counts as 0) — never an error.  Up to 8 vectors per call; an index list (the positions of a compress, the ancestors
    of a resample) can be carried to any number of vectors by further calls.  Filtration time: the later of the index's and the vector's."""
    i_time, ix = _argument(index, "gather")
    args = [_argument(v, "gather") for v in values]
    _check_count("gather", len(args), 1)
    n = args[0][1].n
    for _, v in args:
        if v.n != n: raise ValueError("gather: value vectors of different size")
    times = [max(i_time, t) for t, _ in args]
    if not device_select():
        outs = gather_host(ix.to_float32(), [v.to_float32() for _, v in args])
        return [RandomVariableHip(t, DeviceVector.from_host(o)) for t, o in zip(times, outs)]
    hv = (C.c_int64 * len(args))(*[v.handle for _, v in args])
    out = (C.c_int64 * len(args))()
    N.check(N.lib().fmhip_gather(ix.handle, hv, len(args), out))
    return [RandomVariableHip(t, DeviceVector(int(out[i]), ix.n)) for i, t in enumerate(times)]
