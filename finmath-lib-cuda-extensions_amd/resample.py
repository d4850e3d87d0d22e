"""Resampling on the device (include/fmhip.h: fmhip_resample, fmhip_resample_host): the step that follows the weighted
sample of prefix.py — the weighted sample becomes an equally weighted one without a vector leaving the device.  m ancestors a_j are drawn
from the weights and the state vectors are carried along, out[i][j] = values[i][a_j], bit for bit: a particle filter's resampling step,
importance sampling with weight degeneracy, the bootstrap (equal weights), one draw of ancestors for up to 8 state vectors.

The definition is csrc/resample_host.hpp, one header for the host and the device: weights that are not positive (a NaN, a negative weight,
-0.0) count as zero; P is prefix.prefix_sums_host's P of the cleaned weights, total = P[n-1]; the target of output j is t_j = f_j·total with
f_j = (j + offset)/m (systematic, ONE offset in [0, 1)), (j + U_j)/m (stratified) or U_j (multinomial, in the order of the uniforms); the
ancestor is the smallest r with P[r] > t_j (the smallest r with P[r] == total if rounding at the top leaves none).  A path of zero weight is
never an ancestor.  A total that is not positive or not finite gives NaN everywhere (and ancestors -1 on the host, NaN on the device); a NaN
uniform gives NaN in its element.

FMHIP_DEVICE_RESAMPLE=0, read per call: the A/B switch and the fallback — the vectors are downloaded, fmhip_resample_host (the definition)
runs on one core, and the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

MAX_VALUES = 8
MAX_ANCESTOR_N = 1 << 24
SYSTEMATIC, STRATIFIED, MULTINOMIAL = 0, 1, 2
_SCHEMES = {"systematic": SYSTEMATIC, "stratified": STRATIFIED, "multinomial": MULTINOMIAL}
_pf = C.POINTER(C.c_float)


def device_resample() -> bool:
    """FMHIP_DEVICE_RESAMPLE=0: resamples download their vectors, run the definition on the host and upload the results (the A/B switch and
    the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_RESAMPLE", "1") != "0"


def _scheme(scheme) -> int:
    if isinstance(scheme, str):
        if scheme not in _SCHEMES: raise ValueError(f"resample: scheme {scheme!r} (systematic, stratified or multinomial)")
        return _SCHEMES[scheme]
    return int(scheme)


def _argument(v, what):
    """(time, DeviceVector): a RandomVariableHip keeps its filtration time; a bare DeviceVector has none (-inf)."""
    if isinstance(v, RandomVariableHip):
        if v.isDeterministic(): raise ValueError(f"{what}: a deterministic random variable has no vector to resample")
        return v.time, v.realizations
    if isinstance(v, DeviceVector):
        return -math.inf, v
    raise TypeError(f"{what}: of a RandomVariableHip or a DeviceVector, not {type(v).__name__}")


def _floats(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).ravel()


def resample_host(weights, values, m=None, scheme="systematic", offset=None, uniforms=None):
    """The DEFINITION (fmhip_resample_host) over numpy arrays; needs no device.  weights: n floats or None (equal weights); values: a list
    of up to 8 arrays of n floats.  Returns (outs, ancestors, total): one float32 array of m elements per value vector, the ancestors as
    int64 (-1: a dead element; None where n > 2^24), and the total weight."""
    w = _floats(weights)
    values = [_floats(v) for v in values]
    u = _floats(uniforms)
    n = w.size if w is not None else (values[0].size if values else 0)
    for v in values:
        if v.size != n: raise ValueError("resample: a value vector whose size is not the sample's")
    scheme = _scheme(scheme)
    if m is None: m = u.size if (u is not None and scheme != SYSTEMATIC) else n
    m = int(m)
    if u is not None and scheme != SYSTEMATIC and u.size != m: raise ValueError("resample: the uniforms are one per output")
    outs = [np.empty(max(m, 1), dtype=np.float32) for _ in values]
    ancestors = np.empty(max(m, 1), dtype=np.int64) if n <= MAX_ANCESTOR_N else None
    total = C.c_double(0.0)
    vin = (C.c_void_p * max(len(values), 1))(*[v.ctypes.data for v in values])
    vout = (C.c_void_p * max(len(values), 1))(*[o.ctypes.data for o in outs])
    N.check(N.lib().fmhip_resample_host(None if w is None else w.ctypes.data_as(C.c_void_p), n, scheme, m, 0.0 if offset is None else float(offset),
                                        None if u is None else u.ctypes.data_as(C.c_void_p), vin if values else None, len(values), vout if values else None,
                                        None if ancestors is None else ancestors.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(total)))
    return [o[:m] for o in outs], (None if ancestors is None else ancestors[:m]), total.value


def resample(weights, values, m=None, scheme="systematic", offset=None, uniforms=None, ancestors=False):
    """Draw m ancestors from `weights` (None: equal weights) and carry `values` — up to 8 vectors of the weights' size — along.  Returns
    (outs, total), or (outs, ancestors, total) with ancestors=True: outs[i][j] = values[i][a_j] bit for bit as RandomVariableHip of m
    paths, the ancestors (float32, exact for n <= 2^24; NaN for a dead element) as one more, and the total weight as a float — not positive
    or infinite where every output is NaN.  m defaults to the number of uniforms, or to n.  scheme "systematic" needs ONE offset in [0, 1),
    "stratified" and "multinomial" m uniforms (a vector; below 0 taken as 0, at or above 1 as the largest double below 1).
    Filtration time: an output has the later of the weights' time and its value vector's, as nested.repeat_each keeps its argument's (a
    bare DeviceVector has none); the ancestors have the weights'."""
    scheme = _scheme(scheme)
    w_time, w = (-math.inf, None) if weights is None else _argument(weights, "resample")
    args = [_argument(v, "resample") for v in values]
    if len(args) > MAX_VALUES: raise ValueError(f"resample of {len(args)} value vectors: at most {MAX_VALUES} in one call")
    if w is None and not args: raise ValueError("resample: neither weights nor a value vector")
    if not args and not ancestors: raise ValueError("resample: nothing asked for")
    n = w.n if w is not None else args[0][1].n
    for _, v in args:
        if v.n != n: raise ValueError("resample: a value vector whose size is not the sample's")
    u = None
    if scheme != SYSTEMATIC:
        if uniforms is None: raise ValueError("resample: this scheme needs uniforms")
        _, u = _argument(uniforms, "resample")
    else:
        if offset is None: raise ValueError("resample: the systematic scheme needs an offset in [0, 1)")
        offset = float(offset)
        if not 0.0 <= offset < 1.0: raise ValueError("resample: the offset is in [0, 1)")
    if m is None: m = u.n if u is not None else n
    m = int(m)
    if u is not None and u.n != m: raise ValueError("resample: the uniforms are one per output")
    if ancestors and n > MAX_ANCESTOR_N: raise ValueError("resample: the ancestors are offered up to 2^24 elements, where the float is exact")
    times = [max(w_time, t) for t, _ in args]
    if not device_resample():
        outs, anc, total = resample_host(None if w is None else w.to_float32(), [v.to_float32() for _, v in args], m, scheme, offset,
                                         None if u is None else u.to_float32())
        made = [RandomVariableHip(t, DeviceVector.from_host(o)) for t, o in zip(times, outs)]
        if not ancestors: return made, total
        a = np.where(anc >= 0, anc, np.nan).astype(np.float32)
        return made, RandomVariableHip(w_time, DeviceVector.from_host(a)), total
    hv = (C.c_int64 * max(len(args), 1))(*[v.handle for _, v in args])
    out_values = (C.c_int64 * max(len(args), 1))()
    out_ancestors = C.c_int64(0)
    total = C.c_double(0.0)
    N.check(N.lib().fmhip_resample(0 if w is None else w.handle, scheme, m, 0.0 if offset is None else offset, 0 if u is None else u.handle,
                                   hv if args else None, len(args), out_values if args else None, C.byref(out_ancestors) if ancestors else None, C.byref(total)))
    made = [RandomVariableHip(t, DeviceVector(int(out_values[i]), m)) for i, t in enumerate(times)]
    if not ancestors: return made, total.value
    return made, RandomVariableHip(w_time, DeviceVector(out_ancestors.value, m)), total.value


def systematic_resample(weights, values, offset, m=None, ancestors=False):
    """resample with f_j = (j + offset) / m: ONE uniform for the whole draw, every path's offspring count is floor or ceil of m·w/total."""
    return resample(weights, values, m=m, scheme=SYSTEMATIC, offset=offset, ancestors=ancestors)


def stratified_resample(weights, values, uniforms, ancestors=False):
    """resample with f_j = (j + U_j) / m: one uniform per stratum."""
    return resample(weights, values, scheme=STRATIFIED, uniforms=uniforms, ancestors=ancestors)


def multinomial_resample(weights, values, uniforms, ancestors=False):
    """resample with f_j = U_j: independent draws, in the order of the uniforms."""
    return resample(weights, values, scheme=MULTINOMIAL, uniforms=uniforms, ancestors=ancestors)


def bootstrap_resample(values, uniforms) -> list:
    """The bootstrap: out[i][j] = values[i][min(floor(U_j·n), n - 1)] — equal weights, independent draws, nothing summed or searched."""
    return resample(None, values, scheme=MULTINOMIAL, uniforms=uniforms)[0]


def effective_sample_size(weights) -> float:
    """(Σw)² / Σw² from ONE reduce_moments call; n for equal weights, 1 for one dominant weight.  (The weights as they are: the moments
    know no cleaning.)"""
    _, w = _argument(weights, "effective_sample_size")
    mo = w.moments()
    return mo.sum * mo.sum / mo.sumsq
