"""Tabulated functions on the device (include/fmhip.h: fmhip_table_build, fmhip_table_apply, fmhip_table_apply_host):
RandomVariable.apply for a CURVE — a function tabulated on knots and interpolated: a local-volatility slice σ(t_i, S), a Markov-functional
numéraire as a function of the state, a piecewise-linear payoff profile, an exercise boundary, the inverse CDF of an empirical marginal —
without the vector leaving the device.  An arbitrary lambda cannot run there; a table can.

The definition is host/tabulated_function.hpp, one header that the host and the kernel both compile: X = (double)x, s = the number of knots
<= X, t = X − knots[max(s − 1, 0)], (float)(((C3·t + C2)·t + C1)·t + C0) with every operation rounded on its own in fp64.  The device's
bits are those of fmhip_table_apply_host.  The interpolation names follow finmath-lib's RationalFunctionInterpolation as remembered.

FMHIP_DEVICE_TABLE=0, read per call: the A/B switch and the fallback — the vector is downloaded, fmhip_table_apply_host (the definition)
runs on one core, and the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector

MAX_KNOTS = 1024
MAX_FUNCTIONS = 4
MAX_ENTRIES = 1024
INTERPOLATION = {"piecewise_constant": 0, "linear": 1, "cubic_spline": 2, "monotone_cubic": 3}
EXTRAPOLATION = {"constant": 0, "linear": 1}

_pd = C.POINTER(C.c_double)


def device_table() -> bool:
    """FMHIP_DEVICE_TABLE=0: table_apply downloads the vector, runs the definition on the host and uploads the results (the A/B switch and
    the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_TABLE", "1") != "0"


class TabulatedFunction:
    """A function given by its values at strictly increasing knots (1 … 1024 of them), interpolated ("piecewise_constant", "linear",
    "cubic_spline": natural, "monotone_cubic": Fritsch–Carlson) and extrapolated ("constant", or "linear": value and slope of the adjacent
    segment at the end knot).  .coefficients: (len(knots) + 1, 4) float64, the segments of the definition."""

    def __init__(self, knots, values, interpolation: str = "linear", extrapolation: str = "constant", _derivative: int = 0):
        if interpolation not in INTERPOLATION: raise ValueError(f"interpolation {interpolation!r} (one of {sorted(INTERPOLATION)})")
        if extrapolation not in EXTRAPOLATION: raise ValueError(f"extrapolation {extrapolation!r} (one of {sorted(EXTRAPOLATION)})")
        self.knots = np.ascontiguousarray(knots, dtype=np.float64).ravel().copy()
        self.values = np.ascontiguousarray(values, dtype=np.float64).ravel().copy()
        if self.knots.size != self.values.size: raise ValueError(f"{self.knots.size} knots and {self.values.size} values")
        self.interpolation, self.extrapolation, self.order = interpolation, extrapolation, int(_derivative)
        self.coefficients = np.empty((self.knots.size + 1, 4), dtype=np.float64)
        N.check(N.lib().fmhip_table_build(self.knots.ctypes.data_as(_pd), self.values.ctypes.data_as(_pd), self.knots.size, INTERPOLATION[interpolation],
                                          EXTRAPOLATION[extrapolation], self.order, self.coefficients.ctypes.data_as(_pd)))

    def derivative(self) -> "TabulatedFunction":
        """The derivative of the interpolant, on the same knots: the segments (C1, 2·C2, 3·C3, 0)."""
        if self.order != 0: raise ValueError("the derivative of a derivative is not tabulated")
        return TabulatedFunction(self.knots, self.values, self.interpolation, self.extrapolation, _derivative=1)

    def __call__(self, x: float) -> float:
        """The definition's polynomial at the double x, not narrowed to fp32."""
        X = float(x)
        if X != X: return float("nan")
        s = int(np.searchsorted(self.knots, X, side="right"))
        c0, c1, c2, c3 = (float(c) for c in self.coefficients[s])
        if c1 == 0.0 and c2 == 0.0 and c3 == 0.0: return c0
        t = X - float(self.knots[max(s - 1, 0)])
        return ((c3 * t + c2) * t + c1) * t + c0


def _tables(functions):
    if isinstance(functions, TabulatedFunction): functions = [functions]
    functions = list(functions)
    if not 1 <= len(functions) <= MAX_FUNCTIONS: raise ValueError(f"table_apply: {len(functions)} functions (1 … {MAX_FUNCTIONS} in one call)")
    knots = functions[0].knots
    for f in functions[1:]:
        if f.knots.shape != knots.shape or (f.knots != knots).any(): raise ValueError("table_apply: the functions of one call share their knots")
    if knots.size * len(functions) > MAX_ENTRIES: raise ValueError(f"table_apply: {knots.size} knots x {len(functions)} functions exceed {MAX_ENTRIES}")
    return knots, np.ascontiguousarray(np.stack([f.coefficients for f in functions]))


def table_apply_host(x, functions) -> list:
    """The DEFINITION (fmhip_table_apply_host): one float32 array per function for a host array; needs no device."""
    knots, coef = _tables(functions)
    a = np.ascontiguousarray(x, dtype=np.float32).ravel()
    out = [np.empty(a.size, dtype=np.float32) for _ in range(coef.shape[0])]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    N.check(N.lib().fmhip_table_apply_host(a.ctypes.data_as(C.c_void_p), a.size, knots.ctypes.data_as(_pd), knots.size, coef.ctypes.data_as(_pd), len(out), cols))
    return out


def table_apply(x, functions) -> list:
    """[f(x) for f in functions] as new DeviceVectors from ONE launch that reads x once; 1 … 4 functions on identical knots."""
    v = getattr(x, "realizations", x)
    if not isinstance(v, DeviceVector): raise TypeError("table_apply: of a device vector (or a stochastic RandomVariableHip)")
    knots, coef = _tables(functions)
    if not device_table():
        return [DeviceVector.from_host(o) for o in table_apply_host(v.to_float32(), functions)]
    out = (C.c_int64 * coef.shape[0])()
    N.check(N.lib().fmhip_table_apply(v.handle, knots.ctypes.data_as(_pd), knots.size, coef.ctypes.data_as(_pd), coef.shape[0], out))
    return [DeviceVector(int(h), v.n) for h in out]
