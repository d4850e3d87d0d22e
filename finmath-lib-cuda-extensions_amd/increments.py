"""Independent increments with a law per (time step, factor), drawn from finmath-lib's MT19937 stream through an inverse cumulative
distribution function — mirrors of net.finmath.montecarlo.IndependentIncrementsFromICDF and JumpProcessIncrements, the classes
finmath-lib's jump models (MonteCarloMertonModel, Bates) are built on [unverified: finmath-lib is not vendored; class names, the draw
order and the three-factor layout are restated from its documentation, as everything in host/mersenne.hpp is].

One ``MersenneTwister.nextDouble()`` per increment, path-major (path, step, factor); the law of an increment is chosen by
``laws(time_index, factor)``:

    NormalLaw(scale)        inverse normal CDF (AS 241) times ``scale``: ``sqrt(dt)`` for a Brownian factor, 1 for a jump size
    UniformLaw(lo, hi)      ``lo + (hi - lo) * u``
    PoissonLaw(mean)        ``min { k : F[k] >= u }`` over a CDF table built on the host in fp64, ``0 <= mean <= 128``
    GammaLaw(shape, scale)  inverse regularised incomplete gamma function times ``scale``, ``0.01 <= shape <= 1000``
    ExponentialLaw(rate)    ``-log(1 - u) / rate``

The increments are generated on the device (``fmhip_increments_generate_device``: every workgroup enters the one stream by jump-ahead)
to the bits of the host definition ``fmhip_increments_host`` (host/increments.hpp): Poisson and uniform draws are equal, normal draws
are under the contract of the Mersenne-Twister Brownian motion; gamma and exponential draws are equal too: their
definition (host/gamma_icdf.hpp) is one text for the host and the device, without a library transcendental (§4.11).  ``GammaProcess`` and
``VarianceGammaProcess`` are the pure-jump Lévy processes finmath-lib builds on these increments.  With ``FMHIP_DEVICE_INCREMENTS=0`` — or with a
factory that is not the device's — they are drawn by the host definition and handed to the factory (double[] → fp32): the A/B switch,
and the definition.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip, RandomVariableHipFactory

LAW_NORMAL, LAW_UNIFORM, LAW_POISSON = 0, 1, 2
LAW_GAMMA, LAW_EXPONENTIAL = 4, 5               # 3 is no law


class _Law:
    __slots__ = ("kind", "a", "b")

    def __init__(self, kind, a, b=0.0):
        self.kind, self.a, self.b = int(kind), float(a), float(b)

    def __eq__(self, o): return isinstance(o, _Law) and (self.kind, self.a, self.b) == (o.kind, o.a, o.b)
    def __hash__(self): return hash((self.kind, self.a, self.b))
    def __repr__(self): return f"{type(self).__name__}({self.a}" + (f", {self.b})" if self.kind in (LAW_UNIFORM, LAW_GAMMA) else ")")


class NormalLaw(_Law):
    def __init__(self, scale=1.0): super().__init__(LAW_NORMAL, scale)


class UniformLaw(_Law):
    def __init__(self, lo=0.0, hi=1.0): super().__init__(LAW_UNIFORM, lo, hi)


class PoissonLaw(_Law):
    def __init__(self, mean): super().__init__(LAW_POISSON, mean)


class GammaLaw(_Law):
    def __init__(self, shape, scale=1.0): super().__init__(LAW_GAMMA, shape, scale)


class ExponentialLaw(_Law):
    def __init__(self, rate=1.0): super().__init__(LAW_EXPONENTIAL, rate)


def _device_increments():
    """FMHIP_DEVICE_INCREMENTS=0: the increments are drawn by the host definition on one core and uploaded through the factory (the A/B
    switch); anything else: they are generated on the device (fmhip_increments_generate_device)."""
    return os.environ.get("FMHIP_DEVICE_INCREMENTS", "1") != "0"


def _law_arrays(laws, n_steps, n_factors):
    table = [[laws(i, f) for f in range(n_factors)] for i in range(n_steps)] if callable(laws) else laws
    kinds = np.array([[law.kind for law in row] for row in table], dtype=np.int32).reshape(n_steps * n_factors)
    a = np.array([[law.a for law in row] for row in table], dtype=np.float64).reshape(n_steps * n_factors)
    b = np.array([[law.b for law in row] for row in table], dtype=np.float64).reshape(n_steps * n_factors)
    return kinds, a, b


def _ptrs(kinds, a, b):
    return kinds.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double))


def host_increments(seed, laws, n_steps, n_factors, n_paths):
    """Host array [step][factor][path] (float64) of the increments by the definition, fmhip_increments_host; no device needed.
    ``laws``: a callable (time_index, factor) -> law, or a nested list [step][factor] of laws."""
    kinds, a, b = _law_arrays(laws, n_steps, n_factors)
    out = np.empty((n_steps, n_factors, n_paths), dtype=np.float64)
    N.check(N.lib().fmhip_increments_host(int(seed), n_steps, n_factors, n_paths, *_ptrs(kinds, a, b), out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


class IndependentIncrementsFromICDF:
    """``laws(time_index, factor)`` names the law of increment (time_index, factor).  Method set of BrownianMotionHip; the increments are
    generated on first access and carry the filtration time t_{i+1}.  ``path_offset``: this object holds paths path_offset …
    path_offset + numberOfPaths of the whole process (a rank's block), on either path."""

    def __init__(self, time_discretization, number_of_factors, number_of_paths, seed, laws,
                 random_variable_factory=None, path_offset=0):
        self.timeDiscretization = time_discretization
        self.numberOfFactors = int(number_of_factors)
        self.numberOfPaths = int(number_of_paths)
        self.seed = int(seed)
        self.laws = laws
        self.pathOffset = int(path_offset)
        self.randomVariableFactory = random_variable_factory or RandomVariableHipFactory()
        self._increments = None
        self._lock = threading.Lock()

    def _law_table(self):
        return tuple(tuple(self.laws(i, f) for f in range(self.numberOfFactors)) for i in range(self.timeDiscretization.getNumberOfTimeSteps()))

    def getCloneWithModifiedSeed(self, seed):
        return IndependentIncrementsFromICDF(self.timeDiscretization, self.numberOfFactors, self.numberOfPaths, seed, self.laws,
                                             self.randomVariableFactory, self.pathOffset)

    def getCloneWithModifiedTimeDiscretization(self, new_time_discretization):
        return IndependentIncrementsFromICDF(new_time_discretization, self.numberOfFactors, self.numberOfPaths, self.seed, self.laws,
                                             self.randomVariableFactory, self.pathOffset)

    def getIncrement(self, time_index, factor):
        with self._lock:
            if self._increments is None:
                self._generate()
        return self._increments[time_index][factor]

    def getBrownianIncrement(self, time_index, factor):
        """So that a driver written against BrownianMotion (black_scholes_call_mc) can be fed a normal factor of these increments."""
        return self.getIncrement(time_index, factor)

    def _generate(self):
        td = self.timeDiscretization
        n_steps, n_factors, n = td.getNumberOfTimeSteps(), self.numberOfFactors, self.numberOfPaths
        table = self._law_table()
        if _device_increments() and isinstance(self.randomVariableFactory, RandomVariableHipFactory):
            kinds, a, b = _law_arrays(table, n_steps, n_factors)
            handles = (C.c_int64 * (n_steps * n_factors))()
            N.check(N.lib().fmhip_increments_generate_device(self.seed, n_steps, n_factors, n, self.pathOffset, *_ptrs(kinds, a, b), handles))
            self._increments = [[RandomVariableHip(td.getTime(i + 1), DeviceVector(handles[i * n_factors + f], n)) for f in range(n_factors)]
                                for i in range(n_steps)]
        else:                                   # the host stream is sequential: everything in front of the block is drawn, the block handed over
            block = host_increments(self.seed, table, n_steps, n_factors, self.pathOffset + n)[:, :, self.pathOffset:]
            self._increments = [[self.randomVariableFactory.createRandomVariable(td.getTime(i + 1), np.ascontiguousarray(block[i, f]))
                                 for f in range(n_factors)] for i in range(n_steps)]

    def getTimeDiscretization(self): return self.timeDiscretization
    def getNumberOfFactors(self): return self.numberOfFactors
    def getNumberOfPaths(self): return self.numberOfPaths
    def getSeed(self): return self.seed
    def getRandomVariableForConstant(self, value): return self.randomVariableFactory.createRandomVariable(value)

    def __eq__(self, o):
        return (isinstance(o, IndependentIncrementsFromICDF) and self.numberOfFactors == o.numberOfFactors
                and self.numberOfPaths == o.numberOfPaths and self.seed == o.seed and self.pathOffset == o.pathOffset
                and self.timeDiscretization == o.timeDiscretization and self._law_table() == o._law_table())

    def __hash__(self):
        r = hash(self.timeDiscretization)
        for v in (self.numberOfFactors, self.numberOfPaths, self.seed, hash(self._law_table())):
            r = (31 * r + v) & 0xFFFFFFFF
        return r

    def __repr__(self):
        return (f"{type(self).__name__}(steps={self.timeDiscretization.getNumberOfTimeSteps()}, numberOfPaths={self.numberOfPaths}, "
                f"numberOfFactors={self.numberOfFactors}, seed={self.seed})")


class JumpProcessIncrements(IndependentIncrementsFromICDF):
    """Factor f is a Poisson jump count with mean ``jump_intensities[f] * dt_i`` over time step i."""

    def __init__(self, time_discretization, jump_intensities, number_of_paths, seed, random_variable_factory=None, path_offset=0):
        self.jumpIntensities = tuple(float(v) for v in jump_intensities)

        def laws(time_index, factor):
            return PoissonLaw(self.jumpIntensities[factor] * self.timeDiscretization.getTimeStep(time_index))
        super().__init__(time_discretization, len(self.jumpIntensities), number_of_paths, seed, laws, random_variable_factory, path_offset)

    def getCloneWithModifiedSeed(self, seed):
        return JumpProcessIncrements(self.timeDiscretization, self.jumpIntensities, self.numberOfPaths, seed, self.randomVariableFactory, self.pathOffset)

    def getCloneWithModifiedTimeDiscretization(self, new_time_discretization):
        return JumpProcessIncrements(new_time_discretization, self.jumpIntensities, self.numberOfPaths, self.seed, self.randomVariableFactory, self.pathOffset)


def merton_increments(time_discretization, number_of_paths, seed, jump_intensity, random_variable_factory=None, path_offset=0):
    """The three factors of a Merton jump-diffusion: factor 0 a Brownian increment (normal, sqrt(dt)), factor 1 a standard normal jump
    size, factor 2 a Poisson jump count with mean ``jump_intensity * dt`` [unverified: the layout of finmath-lib's MonteCarloMertonModel]."""
    td = time_discretization

    def laws(i, f):
        if f == 0: return NormalLaw(math.sqrt(td.getTimeStep(i)))
        if f == 1: return NormalLaw(1.0)
        return PoissonLaw(jump_intensity * td.getTimeStep(i))
    return IndependentIncrementsFromICDF(td, 3, number_of_paths, seed, laws, random_variable_factory, path_offset)


class GammaProcess(IndependentIncrementsFromICDF):
    """One factor: the increment over time step i is Gamma(shape_per_time · dt_i, scale) — mean shape_per_time · scale · dt_i.  With
    shape_per_time = 1/ν and scale = ν it is the gamma clock of a variance-gamma process [unverified: finmath-lib's GammaProcess
    (timeDiscretization, numberOfPaths, seed, shape, scale)]."""

    def __init__(self, time_discretization, number_of_paths, seed, shape_per_time, scale=1.0, random_variable_factory=None, path_offset=0):
        self.shapePerTime, self.scale = float(shape_per_time), float(scale)

        def laws(time_index, factor):
            return GammaLaw(self.shapePerTime * self.timeDiscretization.getTimeStep(time_index), self.scale)
        super().__init__(time_discretization, 1, number_of_paths, seed, laws, random_variable_factory, path_offset)

    def getCloneWithModifiedSeed(self, seed):
        return GammaProcess(self.timeDiscretization, self.numberOfPaths, seed, self.shapePerTime, self.scale, self.randomVariableFactory, self.pathOffset)

    def getCloneWithModifiedTimeDiscretization(self, new_time_discretization):
        return GammaProcess(new_time_discretization, self.numberOfPaths, self.seed, self.shapePerTime, self.scale, self.randomVariableFactory, self.pathOffset)


class VarianceGammaProcess:
    """Increments θ·Γ_i + σ·sqrt(Γ_i)·Z_i of a variance-gamma process: a Brownian motion with drift θ and volatility σ run on a gamma
    clock Γ_i ~ Gamma(dt_i/ν, ν).  Γ_i is factor 0 and Z_i (standard normal) factor 1 of ONE IndependentIncrementsFromICDF — one stream, one
    launch — combined with RandomVariable methods, so that the fusion front-end sees the combination [unverified: the factor layout is
    this project's, as the Merton layout is].  One factor towards its callers; ``getGammaIncrement`` hands out the clock."""

    def __init__(self, time_discretization, number_of_paths, seed, sigma, theta, nu, random_variable_factory=None, path_offset=0):
        self.sigma, self.theta, self.nu = float(sigma), float(theta), float(nu)
        td = time_discretization

        def laws(i, f):
            return GammaLaw(td.getTimeStep(i) / self.nu, self.nu) if f == 0 else NormalLaw(1.0)
        self.increments = IndependentIncrementsFromICDF(td, 2, number_of_paths, seed, laws, random_variable_factory, path_offset)
        self._combined = {}
        self._lock = threading.Lock()

    def getGammaIncrement(self, time_index): return self.increments.getIncrement(time_index, 0)

    def getIncrement(self, time_index, factor=0):
        if factor != 0: raise IndexError("a variance-gamma process has one factor")
        with self._lock:
            if time_index not in self._combined:
                g, z = self.increments.getIncrement(time_index, 0), self.increments.getIncrement(time_index, 1)
                self._combined[time_index] = g.mult(self.theta).addProduct(g.sqrt().mult(z), self.sigma)
            return self._combined[time_index]

    def getBrownianIncrement(self, time_index, factor=0): return self.getIncrement(time_index, factor)

    def getCloneWithModifiedSeed(self, seed):
        i = self.increments
        return VarianceGammaProcess(i.timeDiscretization, i.numberOfPaths, seed, self.sigma, self.theta, self.nu, i.randomVariableFactory, i.pathOffset)

    def getCloneWithModifiedTimeDiscretization(self, new_time_discretization):
        i = self.increments
        return VarianceGammaProcess(new_time_discretization, i.numberOfPaths, i.seed, self.sigma, self.theta, self.nu, i.randomVariableFactory, i.pathOffset)

    def getTimeDiscretization(self): return self.increments.getTimeDiscretization()
    def getNumberOfFactors(self): return 1
    def getNumberOfPaths(self): return self.increments.getNumberOfPaths()
    def getSeed(self): return self.increments.getSeed()
    def getRandomVariableForConstant(self, value): return self.increments.getRandomVariableForConstant(value)

    def __eq__(self, o):
        return isinstance(o, VarianceGammaProcess) and (self.sigma, self.theta, self.nu) == (o.sigma, o.theta, o.nu) and self.increments == o.increments

    def __hash__(self): return hash((self.sigma, self.theta, self.nu, hash(self.increments)))

    def __repr__(self):
        return f"VarianceGammaProcess(sigma={self.sigma}, theta={self.theta}, nu={self.nu}, {self.increments!r})"
