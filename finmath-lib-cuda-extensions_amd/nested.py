"""Nested simulation on the device (include/fmhip.h: fmhip_block_moments, fmhip_vec_repeat): the two operations that change
the SHAPE of a sample — k inner paths started from each of m outer states (repeat_each), and the m·k inner payoffs reduced to m
conditional means with their inner variances (block_moments) — without the vectors leaving the device.  With them the primal–dual bounds
of Andersen & Broadie (montecarlo.bermudan_option_bounds_mc), nested exposure and margin simulation, the validation of a regression against
brute-force conditional expectations, batch means and bootstrap blocks run on the device.

A vector of n = m·block elements is m consecutive blocks.  S1 and S2, the fp64 sums of a block's elements and of their exact squares, are
made in ONE association that is a function of `block` alone (host/block_moments.hpp): the device's bits are those of
fmhip_block_moments_host, wherever a block sits and whatever else the call names.

Block order statistics (fmhip_block_order_statistics, fmhip_block_sort; host/block_order.hpp): every block of at most
4096 elements sorted in the order of java.util.Arrays.sort(float[]), and of the sorted block the element at a rank (block_quantiles,
block_min, block_max), the mean over a range of ranks (block_quantile_expectations) or all of it (block_sort) — the quantile, the tail mean
and the worst case per outer path of a nested risk measure (montecarlo.nested_initial_margin_mc).  The device's bits are those of
fmhip_block_order_statistics_host and fmhip_block_sort_host.

FMHIP_DEVICE_NESTED=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition
(fmhip_block_moments_host, fmhip_block_order_statistics_host, fmhip_block_sort_host) or a numpy repeat runs on one core, and the results
are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip, quantile_index

OUTPUTS = {"sum": 1, "mean": 2, "variance": 4}                       # FMHIP_BLOCK_SUM, _MEAN, _VARIANCE
MAX_VECTORS = 4
MAX_N = (1 << 31) - 1
ORDER_MAX_BLOCK, ORDER_MAX_RANKS, ORDER_MAX_RANGES = 4096, 8, 4      # FM_BLOCK_ORDER_MAX, _MAX_RANKS, _MAX_RANGES (host/block_order.hpp)


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


# ---------------------------------------------------------------- block order statistics
def _check_block_length(block, what):
    """FMHIP_ERR_UNSUPPORTED as the library says it, for every kind of operand: a deterministic variable never reaches the library."""
    if block > ORDER_MAX_BLOCK:
        raise N.FmhipError(N.ERR_UNSUPPORTED, f"{what}: blocks of {block} elements (at most {ORDER_MAX_BLOCK}; fmhip_select_ranks_batch selects in whole vectors, "
                                              "fmhip_sort_by_key sorts them)")


def _selectors(block, ranks, ranges):
    block = int(block)
    if block < 1: raise ValueError(f"block_order_statistics: blocks of {block} elements (at least 1)")
    ranks = [int(r) for r in ranks]
    ranges = [(int(a), int(b)) for a, b in ranges]
    if not ranks and not ranges: raise ValueError("block_order_statistics: no rank and no range")
    for r in ranks:
        if not 0 <= r < block: raise ValueError(f"block_order_statistics: rank {r} of a block of {block}")
    for a, b in ranges:
        if not 0 <= a <= b < block: raise ValueError(f"block_order_statistics: range [{a}, {b}] of a block of {block}")
    _check_block_length(block, "block_order_statistics")
    return block, ranks, ranges


def _i64s(values):
    return (C.c_int64 * max(len(values), 1))(*values)


def _selector_groups(ranks, ranges):
    """The selectors in calls of at most 8 ranks and 4 ranges: [(positions of the ranks, positions of the ranges)], every call with one at least."""
    calls = max(-(-len(ranks) // ORDER_MAX_RANKS), -(-len(ranges) // ORDER_MAX_RANGES))
    return [(list(range(c * ORDER_MAX_RANKS, min((c + 1) * ORDER_MAX_RANKS, len(ranks)))),
             list(range(c * ORDER_MAX_RANGES, min((c + 1) * ORDER_MAX_RANGES, len(ranges))))) for c in range(calls)]


def block_order_statistics_host(a, block: int, ranks=(), ranges=()) -> list:
    """The DEFINITION (fmhip_block_order_statistics_host): [one float32 array of a.size / block elements per rank, then per range (from, to)];
    needs no device.  Any number of selectors: they are taken 8 ranks and 4 ranges at a time."""
    ranks, ranges = [int(r) for r in ranks], [(int(f), int(t)) for f, t in ranges]
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    block = int(block)
    m = a.size // block if block >= 1 and a.size % block == 0 else 0
    got_ranks, got_ranges = [None] * len(ranks), [None] * len(ranges)
    for rs, gs in (_selector_groups(ranks, ranges) or [([], [])]):
        out = np.empty((max(len(rs) + len(gs), 1), max(m, 1)), dtype=np.float32)
        N.check(N.lib().fmhip_block_order_statistics_host(a.ctypes.data_as(C.c_void_p), a.size, block, _i64s([ranks[j] for j in rs]), len(rs),
                                                          _i64s([ranges[j][0] for j in gs]), _i64s([ranges[j][1] for j in gs]), len(gs), out.ctypes.data_as(C.c_void_p)))
        for k, j in enumerate(rs): got_ranks[j] = out[k, :m].copy()
        for k, j in enumerate(gs): got_ranges[j] = out[len(rs) + k, :m].copy()
    return got_ranks + got_ranges


def block_sort_host(a, block: int) -> np.ndarray:
    """The DEFINITION (fmhip_block_sort_host): every block of `block` elements in the order of java.util.Arrays.sort(float[]); NaNs come back
    as the quiet NaN.  Needs no device."""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    out = np.empty(max(a.size, 1), dtype=np.float32)
    N.check(N.lib().fmhip_block_sort_host(a.ctypes.data_as(C.c_void_p), a.size, int(block), out.ctypes.data_as(C.c_void_p)))
    return out[:a.size]


def block_order_statistics(vectors, block: int, ranks=(), ranges=()) -> list:
    """[[the element at rank r of every ascending-sorted block for r in ranks] + [the mean of the ranks from … to of it for (from, to) in
    ranges] for v in vectors] as RandomVariableHip of size / block paths.  block <= 4096.  Up to 4 vectors, 8 ranks and 4 ranges per launch;
    more are taken in groups.  A deterministic variable stays deterministic: every order statistic of a constant block is its value."""
    block, ranks, ranges = _selectors(block, ranks, ranges)
    args = [_argument(v, "block_order_statistics") for v in vectors]
    if not args: raise ValueError("block_order_statistics: of no vector")
    n_out = len(ranks) + len(ranges)
    results = [None] * len(args)
    stochastic = [i for i, (_, dv, _) in enumerate(args) if dv is not None]
    for i, (time, dv, value) in enumerate(args):
        if dv is None: results[i] = [RandomVariableHip(time, float(np.float32(value))) for _ in range(n_out)]
    sizes = {args[i][1].n for i in stochastic}
    if len(sizes) > 1: raise ValueError(f"block_order_statistics: vectors of different sizes {sorted(sizes)}")
    if stochastic and next(iter(sizes)) % block != 0: raise ValueError(f"block_order_statistics: {next(iter(sizes))} elements are no whole number of blocks of {block}")
    for at in range(0, len(stochastic), MAX_VECTORS):
        group = stochastic[at:at + MAX_VECTORS]
        m = args[group[0]][1].n // block
        made = [[None] * n_out for _ in group]
        if not device_nested():
            for g, i in enumerate(group):
                made[g] = [DeviceVector.from_host(o) for o in block_order_statistics_host(args[i][1].to_float32(), block, ranks, ranges)]
        else:
            handles = (C.c_int64 * len(group))(*[args[i][1].handle for i in group])
            for rs, gs in _selector_groups(ranks, ranges):
                per = len(rs) + len(gs)
                out = (C.c_int64 * (len(group) * per))()
                N.check(N.lib().fmhip_block_order_statistics(handles, len(group), block, _i64s([ranks[j] for j in rs]), len(rs),
                                                             _i64s([ranges[j][0] for j in gs]), _i64s([ranges[j][1] for j in gs]), len(gs), out))
                for g in range(len(group)):
                    for k, j in enumerate(rs): made[g][j] = DeviceVector(int(out[g * per + k]), m)
                    for k, j in enumerate(gs): made[g][len(ranks) + j] = DeviceVector(int(out[g * per + len(rs) + k]), m)
        for g, i in enumerate(group):
            results[i] = [RandomVariableHip(args[i][0], dv) for dv in made[g]]
    return results


def block_quantiles(v, block: int, quantiles) -> list:
    """[getQuantile(q) of every block for q in quantiles]: the rank is quantile_index(block, q), the convention of getQuantile (the position
    (block + 1)(1 − q) − 1 of the ascending block, rounded and clamped)."""
    return block_order_statistics([v], block, ranks=[quantile_index(int(block), float(q)) for q in quantiles])[0]


def block_quantile_expectations(v, block: int, pairs) -> list:
    """[getQuantileExpectation(start, end) of every block for (start, end) in pairs]: the mean of the ascending block from position
    (block + 1)·start − 1 to (block + 1)·end − 1, both rounded and clamped (a pair in the wrong order is swapped, as the method does)."""
    block = int(block)
    def position(q): return min(max(int(math.floor((block + 1) * q - 1 + 0.5)), 0), block - 1)
    return block_order_statistics([v], block, ranges=[(position(min(a, b)), position(max(a, b))) for a, b in pairs])[0]


def block_min(v, block: int) -> RandomVariableHip:
    """The smallest element of every block (−0.0 before +0.0; a block of NaNs alone gives NaN)."""
    return block_order_statistics([v], block, ranks=[0])[0][0]


def block_max(v, block: int) -> RandomVariableHip:
    """The largest element of every block in the order of Arrays.sort: a NaN, if the block holds one."""
    return block_order_statistics([v], block, ranks=[int(block) - 1])[0][0]


def block_sort(v, block: int) -> RandomVariableHip:
    """Every block of `block` (<= 4096) consecutive elements sorted ascending, as one new variable of the same size.  NaNs come back as the
    quiet NaN; keys are carried, not paths: sort_by_key is the stable, payload-preserving sort.  A deterministic variable stays one."""
    block = int(block)
    if block < 1: raise ValueError(f"block_sort: blocks of {block} elements (at least 1)")
    _check_block_length(block, "block_sort")
    time, dv, value = _argument(v, "block_sort")
    if dv is None: return RandomVariableHip(time, value)
    if dv.n % block != 0: raise ValueError(f"block_sort: {dv.n} elements are no whole number of blocks of {block}")
    if not device_nested():
        return RandomVariableHip(time, DeviceVector.from_host(block_sort_host(dv.to_float32(), block)))
    h = C.c_int64(0)
    N.check(N.lib().fmhip_block_sort(dv.handle, block, C.byref(h)))
    return RandomVariableHip(time, DeviceVector(h.value, dv.n))
