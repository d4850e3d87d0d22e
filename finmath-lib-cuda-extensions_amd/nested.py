"""Nested simulation on the device (include/fmhip.h: fmhip_block_moments, fmhip_vec_repeat): the two operations that change
the SHAPE of a sample — k inner paths started from each of m outer states (repeat_each), and the m·k inner payoffs reduced to m
conditional means with their inner variances (block_moments) — without the vectors leaving the device.  With them the primal–dual bounds
of Andersen & Broadie (montecarlo.bermudan_option_bounds_mc), nested exposure and margin simulation, the validation of a regression against
brute-force conditional expectations, batch means and bootstrap blocks run on the device.

A vector of n = m·block elements is m consecutive blocks.  S1 and S2, the fp64 sums of a block's elements and of their exact squares, are
made in ONE association that is a function of `block` alone (host/block_moments.hpp): the device's bits are those of
fmhip_block_moments_host, wherever a block sits and whatever else the call names.

FMHIP_DEVICE_NESTED=0, read per call: the A/B switch and the fallback — the vectors are downloaded, fmhip_block_moments_host (the
definition) or a numpy repeat runs on one core, and the results are uploaded.  The device path never falls back on its own: a missing
kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

OUTPUTS = {"sum": 1, "mean": 2, "variance": 4}                       # FMHIP_BLOCK_SUM, _MEAN, _VARIANCE
MAX_VECTORS = 4
MAX_N = (1 << 31) - 1


def device_nested() -> bool:
    """FMHIP_DEVICE_NESTED=0: block moments and repeats download their vectors, run the definition (resp. numpy's repeat) on the host and
    upload the results (the A/B switch and the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_NESTED", "1") != "0"


def _outputs(outputs):
    if isinstance(outputs, str): outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"block_moments: outputs {outputs!r} (distinct names out of {sorted(OUTPUTS)})")
    mask = sum(OUTPUTS[o] for o in outputs)
    return outputs, mask, [o for o in ("sum", "mean", "variance") if o in outputs]


def _argument(v, what):
    """(time, DeviceVector or None, value): a RandomVariableHip keeps its filtration time; a bare DeviceVector has none (-inf)."""
    if isinstance(v, RandomVariableHip):
        return v.time, v.realizations, v.value
    if isinstance(v, DeviceVector):
        return -math.inf, v, math.nan
    raise TypeError(f"{what}: of a RandomVariableHip or a DeviceVector, not {type(v).__name__}")


def block_moments_host(a, block: int, outputs=("mean",)) -> list:
    """The DEFINITION (fmhip_block_moments_host): [one float32 array of a.size / block elements per name of outputs]; needs no device."""
    outputs, mask, in_bit_order = _outputs(outputs)
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    block = int(block)
    m = a.size // block if block >= 1 and a.size % block == 0 else 0
    out = np.empty((len(outputs), max(m, 1)), dtype=np.float32)
    N.check(N.lib().fmhip_block_moments_host(a.ctypes.data_as(C.c_void_p), a.size, block, mask, out.ctypes.data_as(C.c_void_p)))
    return [out[in_bit_order.index(o)].copy() for o in outputs]


def block_moments(vectors, block: int, outputs=("mean",)) -> list:
    """[[output of v for each name of outputs] for v in vectors] as RandomVariableHip of size / block paths: "sum", "mean" and "variance" (the
    population variance from raw fp64 moments) of the consecutive blocks of `block` elements.  Up to 4 vectors of one size per launch,
    each read once; more are taken four at a time.  A deterministic variable stays deterministic: its block mean is its value."""
    outputs, mask, in_bit_order = _outputs(outputs)
    block = int(block)
    if block < 1: raise ValueError(f"block_moments: blocks of {block} elements (at least 1)")
    args = [_argument(v, "block_moments") for v in vectors]
    if not args: raise ValueError("block_moments: of no vector")
    results = [None] * len(args)
    stochastic = [i for i, (_, dv, _) in enumerate(args) if dv is not None]
    for i, (time, dv, value) in enumerate(args):
        if dv is None:
            constant = {"sum": float(np.float32(np.float64(value) * block)), "mean": float(np.float32(value)), "variance": 0.0}
            results[i] = [RandomVariableHip(time, constant[o]) for o in outputs]
    sizes = {args[i][1].n for i in stochastic}
    if len(sizes) > 1: raise ValueError(f"block_moments: vectors of different sizes {sorted(sizes)}")
    if stochastic and next(iter(sizes)) % block != 0: raise ValueError(f"block_moments: {next(iter(sizes))} elements are no whole number of blocks of {block}")
    for at in range(0, len(stochastic), MAX_VECTORS):
        group = stochastic[at:at + MAX_VECTORS]
        m = args[group[0]][1].n // block
        if not device_nested():
            made = [[DeviceVector.from_host(o) for o in block_moments_host(args[i][1].to_float32(), block, in_bit_order)] for i in group]
        else:
            handles = (C.c_int64 * len(group))(*[args[i][1].handle for i in group])
            out = (C.c_int64 * (len(group) * len(outputs)))()
            N.check(N.lib().fmhip_block_moments(handles, len(group), block, mask, out))
            made = [[DeviceVector(int(out[g * len(outputs) + j]), m) for j in range(len(outputs))] for g in range(len(group))]
        for g, i in enumerate(group):
            results[i] = [RandomVariableHip(args[i][0], made[g][in_bit_order.index(o)]) for o in outputs]
    return results


def block_means(v, block: int) -> RandomVariableHip:
    """The mean of every block of `block` consecutive elements: the conditional mean per outer path of a nested simulation."""
    return block_moments([v], block, ("mean",))[0][0]


def _repeat(v, each: int, times: int, what: str) -> RandomVariableHip:
    each, times = int(each), int(times)
    if each < 1 or times < 1: raise ValueError(f"{what}: {min(each, times)} copies (at least 1)")
    time, dv, value = _argument(v, what)
    if dv is None: return RandomVariableHip(time, value)
    if dv.n * each * times > MAX_N: raise ValueError(f"{what}: an output of {dv.n * each * times} elements (at most 2^31 - 1)")
    if not device_nested():
        a = dv.to_float32()
        return RandomVariableHip(time, DeviceVector.from_host(np.tile(np.repeat(a, each), times)))
    h = C.c_int64(0)
    N.check(N.lib().fmhip_vec_repeat(dv.handle, each, times, C.byref(h)))
    return RandomVariableHip(time, DeviceVector(h.value, dv.n * each * times))


def repeat_each(v, each: int) -> RandomVariableHip:
    """out[p·each + e] = v[p], bit for bit: `each` inner paths per outer state (numpy's repeat).  A deterministic variable stays one."""
    return _repeat(v, each, 1, "repeat_each")


def tile(v, times: int) -> RandomVariableHip:
    """out[t·n + p] = v[p], bit for bit: the sample `times` times in a row (numpy's tile).  A deterministic variable stays one."""
    return _repeat(v, 1, times, "tile")
