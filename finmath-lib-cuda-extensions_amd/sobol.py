"""Quasi-Monte-Carlo: a Sobol' sequence and the Brownian motion built from it with a Brownian bridge — what finmath-lib's
``net.finmath.randomnumbers.SobolSequence`` taken through ``BrownianMotionFromRandomNumberGenerator`` and ``BrownianBridge`` serve
[unverified: finmath-lib is not vendored; names restated from its documentation].

The definition is host/sobol.hpp: Joe & Kuo's direction numbers, 1024 dimensions, Gray-code order with the origin
skipped (path p uses point p + 1), an optional digital shift drawn from MT19937(seed), the inverse normal CDF (AS 241), and per factor
either one dimension per time step (``construction="incremental"``) or a Brownian bridge that spends the first, best dimensions on the
terminal value and the coarse midpoints (``"bridge"``).  The increments are generated on the device (``fmhip_bm_generate_sobol_device``)
and EQUAL the host definition's narrowed to fp32, every one; FMHIP_DEVICE_SOBOL=0 draws them by the host definition and uploads them
through the factory path (the A/B switch).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _native as N
from .brownian_motion import BrownianMotionHip
from .random_variable import DeviceVector, RandomVariableHip

SOBOL_INCREMENTAL, SOBOL_BRIDGE = 0, 1
_CONSTRUCTIONS = {"incremental": SOBOL_INCREMENTAL, "bridge": SOBOL_BRIDGE, SOBOL_INCREMENTAL: SOBOL_INCREMENTAL, SOBOL_BRIDGE: SOBOL_BRIDGE}
SOBOL_MAX_DIMENSION = 1024


def _device_sobol():
    """FMHIP_DEVICE_SOBOL=0: the increments are drawn by the host definition and uploaded (the A/B switch); anything else: they are
    generated on the device (fmhip_bm_generate_sobol_device)."""
    return os.environ.get("FMHIP_DEVICE_SOBOL", "1") != "0"


def _construction(c):
    try:
        return _CONSTRUCTIONS[c]
    except (KeyError, TypeError):
        raise ValueError(f"construction is 'bridge' or 'incremental', not {c!r}") from None


class SobolSequence:
    """Points of the Sobol' sequence in `dimension` <= 1024 dimensions, on the host: ``getNext()`` returns point 1, 2, … (the origin is
    skipped) as `dimension` doubles in (0, 1).  ``seed=None``: the plain sequence; a seed: digitally shifted by MT19937(seed)."""

    def __init__(self, dimension, seed=None):
        self.dimension = int(dimension)
        self.seed = None if seed is None else int(seed)
        self._next = 1
        if not 1 <= self.dimension <= SOBOL_MAX_DIMENSION:
            raise ValueError(f"dimension 1 … {SOBOL_MAX_DIMENSION}")

    def points(self, first_index, count):
        """[count, dimension] float64: the points with indices first_index … first_index + count (index 0 is the origin)."""
        out = np.empty((int(count), self.dimension), dtype=np.float64)
        N.check(N.lib().fmhip_sobol_points_host(self.dimension, int(first_index), int(count), self.seed or 0, 0 if self.seed is None else 1,
                                                out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def getNext(self):
        p = self.points(self._next, 1)[0]
        self._next += 1
        return p

    def getDimension(self): return self.dimension


def sobol_increments(seed, dt, n_factors, n_paths, construction="bridge", randomize=True, path_offset=0):
    """Host array [step][factor][path] (float64) of the increments of paths path_offset … path_offset + n_paths by the definition,
    fmhip_sobol_increments_host; no device needed."""
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    out = np.empty((dt.size, int(n_factors), int(n_paths)), dtype=np.float64)
    N.check(N.lib().fmhip_sobol_increments_host(int(seed), 1 if randomize else 0, _construction(construction), dt.size, int(n_factors), int(n_paths),
                                                int(path_offset), dt.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


class BrownianMotionFromSobolSequence(BrownianMotionHip):
    """A Brownian motion whose increments come from Sobol' points through a Brownian bridge (or increment by increment), generated on the
    device.  number_of_time_steps · number_of_factors <= 1024.  `path_offset`: this object holds paths path_offset … path_offset +
    numberOfPaths of the whole motion — a point is a function of its index, so a rank's block costs what it holds."""

    def __init__(self, time_discretization, number_of_factors, number_of_paths, seed, construction="bridge", randomize=True,
                 random_variable_factory=None, path_offset=0):
        super().__init__(time_discretization, number_of_factors, number_of_paths, seed, random_variable_factory, path_offset)
        self.construction = _construction(construction)
        self.randomize = bool(randomize)

    def getCloneWithModifiedSeed(self, seed):
        return BrownianMotionFromSobolSequence(self.timeDiscretization, self.numberOfFactors, self.numberOfPaths, seed, self.construction,
                                               self.randomize, self.randomVariableFactory, self.pathOffset)

    def getCloneWithModifiedTimeDiscretization(self, new_time_discretization):
        return BrownianMotionFromSobolSequence(new_time_discretization, self.numberOfFactors, self.numberOfPaths, self.seed, self.construction,
                                               self.randomize, self.randomVariableFactory, self.pathOffset)

    def _generate(self):
        td = self.timeDiscretization
        n_steps = td.getNumberOfTimeSteps()
        dt = np.array([td.getTimeStep(i) for i in range(n_steps)], dtype=np.float64)
        count = n_steps * self.numberOfFactors
        handles = (C.c_int64 * count)()
        if _device_sobol():
            N.check(N.lib().fmhip_bm_generate_sobol_device(self.seed, 1 if self.randomize else 0, self.construction, n_steps, self.numberOfFactors,
                                                           self.numberOfPaths, self.pathOffset, dt.ctypes.data_as(C.POINTER(C.c_double)), handles))
        else:
            block = sobol_increments(self.seed, dt, self.numberOfFactors, self.numberOfPaths, self.construction, self.randomize, self.pathOffset)
            block = block.reshape(count, self.numberOfPaths)
            for k in range(count):
                h = C.c_int64(0)
                N.check(N.lib().fmhip_vec_create_from_double(block[k].ctypes.data_as(C.POINTER(C.c_double)), self.numberOfPaths, C.byref(h)))
                handles[k] = h.value
        self._increments = [
            [RandomVariableHip(td.getTime(i + 1), DeviceVector(handles[i * self.numberOfFactors + f], self.numberOfPaths))
             for f in range(self.numberOfFactors)]
            for i in range(n_steps)]

    def __eq__(self, o):
        return (isinstance(o, BrownianMotionFromSobolSequence) and super().__eq__(o) and self.construction == o.construction
                and self.randomize == o.randomize)

    __hash__ = BrownianMotionHip.__hash__

    def __repr__(self):
        return (f"BrownianMotionFromSobolSequence(steps={self.timeDiscretization.getNumberOfTimeSteps()}, numberOfPaths={self.numberOfPaths}, "
                f"numberOfFactors={self.numberOfFactors}, seed={self.seed}, construction={'bridge' if self.construction else 'incremental'}, "
                f"randomize={self.randomize})")
