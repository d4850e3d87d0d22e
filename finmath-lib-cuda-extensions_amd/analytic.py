"""Named functions and option formulas per path on the device (include/fmhip.h: fmhip_function_apply, fmhip_option_formula and their
_host twins): the most common arguments of RandomVariable.apply — the normal distribution function Φ, its density φ, its
quantile Φ⁻¹ — and the closed-form prices built on them (Black–Scholes and Bachelier: value, delta, vega of a call in forward form), on
vectors that already live in HBM: conditional Monte-Carlo, analytic control variates, exposures of options on simulated forwards and
volatilities, Gaussian copulas and normal scores, and adjoint differentiation through all of it.

The definition is host/normal_functions.hpp, one header that the host and the kernels both compile: fp64, + − × /, sqrt and the exp and log
of host/gamma_icdf.hpp, every operation rounded on its own.  The device's bits are those of fmhip_function_apply_host and
fmhip_option_formula_host.  The formulas are finmath-lib's AnalyticFormulas.blackScholesGeneralizedOptionValue / bachelierOptionValue as
remembered, not as read: that class is not part of the reference tree.

The inverse of the formulas' value in the volatility (fmhip_implied_volatility and its _host twin; host/implied_volatility.hpp; DESIGN.md
§4.25) is below them: implied_volatility with its partials in the price and the forward, a put by parity, a strike per path, the conversion
between a lognormal and a normal volatility, and adjoint differentiation through a quoted volatility.

FMHIP_DEVICE_ANALYTIC=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition runs on one core, and
the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import statistics

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

MAX_FUNCTIONS = 4
MODELS = {"black_scholes": 0, "bachelier": 1}
OUTPUTS = {"value": 1, "delta": 2, "vega": 4}

_pi32 = C.POINTER(C.c_int32)
_STANDARD_NORMAL = statistics.NormalDist()


def device_analytic() -> bool:
    """FMHIP_DEVICE_ANALYTIC=0: function_apply and option_formula download their vectors, run the definition on the host and upload the
    results (the A/B switch and the fallback); anything else: on the device.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_ANALYTIC", "1") != "0"


# ---------------------------------------------------------------- the functions at a double
def _cdf(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _density(x: float) -> float:
    return math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi) if not math.isinf(x) else 0.0


def _quantile(u: float) -> float:
    if not 0.0 <= u <= 1.0: return math.nan                                 # a NaN among them
    if u == 0.0: return -math.inf
    if u == 1.0: return math.inf
    return _STANDARD_NORMAL.inv_cdf(u)                                      # AS 241, the algorithm of the definition


class NamedFunction:
    """A function the device knows by NAME (kind = FMHIP_FN_*).  Callable on a double; .derivative() where the derivative is a named
    function (Φ' = φ), None otherwise — the AAD wrapper composes the other derivatives (φ' = −x·φ, (Φ⁻¹)' = 1/φ(Φ⁻¹))."""
    __slots__ = ("name", "kind", "_at", "_derivative")

    def __init__(self, name, kind, at, derivative=None):
        self.name, self.kind, self._at, self._derivative = name, kind, at, derivative

    def __call__(self, x: float) -> float:
        x = float(x)
        return math.nan if x != x else self._at(x)

    def derivative(self):
        return self._derivative

    def __repr__(self):
        return f"NamedFunction({self.name})"


NORMAL_DENSITY = NamedFunction("NORMAL_DENSITY", 1, _density)
NORMAL_CDF = NamedFunction("NORMAL_CDF", 0, _cdf, NORMAL_DENSITY)
NORMAL_QUANTILE = NamedFunction("NORMAL_QUANTILE", 2, _quantile)


def _kinds(functions):
    if isinstance(functions, NamedFunction): functions = [functions]
    functions = list(functions)
    if not 1 <= len(functions) <= MAX_FUNCTIONS: raise ValueError(f"function_apply: {len(functions)} functions (1 … {MAX_FUNCTIONS} in one call)")
    for f in functions:
        if not isinstance(f, NamedFunction): raise TypeError(f"function_apply: {f!r} is not a NamedFunction")
    return np.array([f.kind for f in functions], dtype=np.int32)


def function_apply_host(x, functions) -> list:
    """The DEFINITION (fmhip_function_apply_host): one float32 array per function for a host array; needs no device."""
    kinds = _kinds(functions)
    a = np.ascontiguousarray(x, dtype=np.float32).ravel()
    out = [np.empty(a.size, dtype=np.float32) for _ in range(kinds.size)]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    N.check(N.lib().fmhip_function_apply_host(a.ctypes.data_as(C.c_void_p), a.size, kinds.ctypes.data_as(_pi32), kinds.size, cols))
    return out


def function_apply(x, functions) -> list:
    """[f(x) for f in functions] as new DeviceVectors from ONE launch that reads x once; 1 … 4 named functions ([NORMAL_CDF,
    NORMAL_DENSITY] is the pair a derivative needs)."""
    v = getattr(x, "realizations", x)
    if not isinstance(v, DeviceVector): raise TypeError("function_apply: of a device vector (or a stochastic RandomVariableHip)")
    kinds = _kinds(functions)
    if not device_analytic():
        return [DeviceVector.from_host(o) for o in function_apply_host(v.to_float32(), functions)]
    out = (C.c_int64 * kinds.size)()
    N.check(N.lib().fmhip_function_apply(v.handle, kinds.ctypes.data_as(_pi32), kinds.size, out))
    return [DeviceVector(int(h), v.n) for h in out]


def normal_scores(x) -> DeviceVector:
    """Φ⁻¹ of the empirical-CDF scores (sorting.rank_scores) per path: the normal scores of a sample, for a Gaussian copula or a rank
    correlation that is Pearson's of the scores (van der Waerden).  Strictly finite: the scores lie strictly inside (0, 1)."""
    from .sorting import rank_scores
    return function_apply(rank_scores(x), [NORMAL_QUANTILE])[0]


# ---------------------------------------------------------------- the formulas
def _mask(outputs):
    if isinstance(outputs, str): outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"option_formula: outputs {outputs!r} (distinct names out of {sorted(OUTPUTS)})")
    mask = sum(OUTPUTS[o] for o in outputs)
    in_bit_order = [o for o in ("value", "delta", "vega") if o in outputs]
    return outputs, mask, in_bit_order


def _model(model):
    if model not in MODELS: raise ValueError(f"option_formula: model {model!r} (one of {sorted(MODELS)})")
    return MODELS[model]


def _check_scalars(maturity, strike):
    maturity, strike = float(maturity), float(strike)
    if not (maturity >= 0.0 and math.isfinite(maturity)): raise ValueError("option_formula: the maturity is finite and not negative")
    if not math.isfinite(strike): raise ValueError("option_formula: the strike is finite")
    return maturity, strike


def option_formula_double(model, forward, volatility, maturity, strike, payoff_unit=1.0) -> dict:
    """The formulas at doubles, in double: {"value", "delta", "vega"}.  What a call with deterministic operands returns."""
    m = _model(model)
    T, K = _check_scalars(maturity, strike)
    F, sigma, unit = float(forward), float(volatility), float(payoff_unit)
    if any(v != v for v in (F, sigma, unit)): return {"value": math.nan, "delta": math.nan, "vega": math.nan}
    root_T = math.sqrt(T)
    s = sigma * root_T
    if not (s > 0.0 and (m != 0 or (F > 0.0 and K > 0.0))):
        return {"value": unit * max(F - K, 0.0), "delta": unit * (1.0 if F > K else 0.0), "vega": 0.0}
    if m == 0:
        d_plus = (math.log(F / K) + 0.5 * s * s) / s
        return {"value": unit * (F * _cdf(d_plus) - K * _cdf(d_plus - s)), "delta": unit * _cdf(d_plus), "vega": unit * F * _density(d_plus) * root_T}
    d = (F - K) / s
    return {"value": unit * ((F - K) * _cdf(d) + s * _density(d)), "delta": unit * _cdf(d), "vega": unit * root_T * _density(d)}


def option_formula_host(model, forward, volatility, maturity, strike, payoff_unit=1.0, outputs=("value",)) -> list:
    """The DEFINITION (fmhip_option_formula_host) over host arrays: forward, volatility and payoff_unit are float32 arrays of one size or
    numbers (fp64 scalars), at least one an array; one float32 array per name of `outputs`, in the order given."""
    m = _model(model)
    T, K = _check_scalars(maturity, strike)
    names, mask, in_bit_order = _mask(outputs)
    arrays, scalars, n = [], [], None
    for o in (forward, volatility, payoff_unit):
        if np.isscalar(o):
            arrays.append(None); scalars.append(float(o))
        else:
            a = np.ascontiguousarray(o, dtype=np.float32).ravel()
            if n is not None and a.size != n: raise ValueError("option_formula: arrays of different size")
            n = a.size
            arrays.append(a); scalars.append(0.0)
    if n is None: raise ValueError("option_formula_host: at least one operand is an array (option_formula_double takes numbers)")
    out = [np.empty(n, dtype=np.float32) for _ in in_bit_order]
    cols = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays]
    N.check(N.lib().fmhip_option_formula_host(m, ptr[0], scalars[0], ptr[1], scalars[1], ptr[2], scalars[2], n, T, K, mask, cols))
    by_name = dict(zip(in_bit_order, out))
    return [by_name[o] for o in names]


def _formula_vectors(m, operands, T, K, mask, n_out):
    """fmhip_option_formula on DeviceVectors and floats: n_out new DeviceVectors, in bit order."""
    handles = [o.handle if isinstance(o, DeviceVector) else 0 for o in operands]
    scalars = [0.0 if isinstance(o, DeviceVector) else float(o) for o in operands]
    n = next(o.n for o in operands if isinstance(o, DeviceVector))
    if not device_analytic():
        host = [o.to_float32() if isinstance(o, DeviceVector) else None for o in operands]
        out = [np.empty(n, dtype=np.float32) for _ in range(n_out)]
        cols = (C.c_void_p * n_out)(*[o.ctypes.data for o in out])
        ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in host]
        N.check(N.lib().fmhip_option_formula_host(m, ptr[0], scalars[0], ptr[1], scalars[1], ptr[2], scalars[2], n, T, K, mask, cols))
        return [DeviceVector.from_host(o) for o in out]
    out = (C.c_int64 * n_out)()
    N.check(N.lib().fmhip_option_formula(m, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], T, K, mask, out))
    return [DeviceVector(int(h), n) for h in out]


def _inner_formula(model, operands, T, K, names, inner_factory=None):
    """The formula on plain (not differentiable) operands — RandomVariableHip, numbers, or with inner_factory any RandomVariable with
    getRealizations: {name: RandomVariable} with the maximum filtration time."""
    m = _model(model)
    _, mask, in_bit_order = _mask(names)
    times = [o.getFiltrationTime() for o in operands if not np.isscalar(o)]
    time = max(times) if times else -math.inf
    make = (lambda value: RandomVariableHip(time, value)) if inner_factory is None else (lambda value: inner_factory.createRandomVariable(time, value))
    if all(np.isscalar(o) or o.isDeterministic() for o in operands):
        F, sigma, unit = (float(o) if np.isscalar(o) else o.doubleValue() for o in operands)
        values = option_formula_double(model, F, sigma, T, K, unit)
        return {o: make(values[o]) for o in in_bit_order}
    if inner_factory is None:
        for o in operands:
            if not np.isscalar(o) and not isinstance(o, RandomVariableHip): raise TypeError(f"option_formula: {type(o).__name__} operands need the factory that made them (an AAD wrapper carries it)")
        plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else o.realizations for o in operands]
        return {o: make(v) for o, v in zip(in_bit_order, _formula_vectors(m, plain, T, K, mask, len(in_bit_order)))}
    plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else np.asarray(o.getRealizations(), dtype=np.float32) for o in operands]
    return {o: make(v) for o, v in zip(in_bit_order, option_formula_host(model, plain[0], plain[1], T, K, plain[2], in_bit_order))}


def option_formula(model, forward, volatility, maturity, strike, payoff_unit=1.0, outputs=("value",)):
    """Value, delta (∂/∂forward) and vega (∂/∂volatility) of a CALL in forward form under "black_scholes" or "bachelier", per path: forward,
    volatility and payoff_unit (a discount factor, a notional, an annuity) are RandomVariableHip or numbers, maturity >= 0 and strike are
    numbers.  One launch whatever the outputs; operands stay where they are.  Returns one RandomVariable per name of `outputs`, as a tuple
    in the order given; the filtration time is the operands' maximum.  Deterministic operands give a deterministic result computed in
    double.  An element with σ√T <= 0 (and under Black–Scholes with forward <= 0 or strike <= 0) is the limit: intrinsic value, a step
    delta, vega 0.  A put is the call minus payoff_unit·(forward − strike).

    RandomVariableDifferentiableAAD operands: the formula runs ONCE with payoff unit 1 and all three outputs, the result is multiplied by
    payoff_unit with the recorded operations, and delta and vega are the recorded partials of the value; a "delta" or "vega" asked for is
    payoff_unit times that vector, itself not differentiable further."""
    from .differentiable import RandomVariableDifferentiableAAD, _Node
    T, K = _check_scalars(maturity, strike)
    names, _, _ = _mask(outputs)
    operands = (forward, volatility, payoff_unit)
    if not any(isinstance(o, RandomVariableDifferentiableAAD) for o in operands):
        results = _inner_formula(model, operands, T, K, names)
        return tuple(results[o] for o in names)
    factory = next(o.factory for o in operands if isinstance(o, RandomVariableDifferentiableAAD))
    inner = [o.values if isinstance(o, RandomVariableDifferentiableAAD) else o for o in operands]
    hip = all(np.isscalar(o) or isinstance(o, RandomVariableHip) for o in inner)
    if not hip and factory is None: raise NotImplementedError("option_formula on this inner implementation needs the factory that made the variables")
    unit = _inner_formula(model, (inner[0], inner[1], 1.0), T, K, ("value", "delta", "vega"), None if hip else factory.inner)
    nodes = tuple(o.node if isinstance(o, RandomVariableDifferentiableAAD) else None for o in operands[:2])
    value = RandomVariableDifferentiableAAD(unit["value"], _Node("OPTION_FORMULA", nodes, (unit["delta"], unit["vega"]), 0.0), factory)
    scaled = {"value": value if np.isscalar(payoff_unit) and float(payoff_unit) == 1.0 else value.mult(payoff_unit)}
    for name in ("delta", "vega"):
        if name in names: scaled[name] = RandomVariableDifferentiableAAD(unit[name].mult(inner[2]), None, factory)
    return tuple(scaled[o] for o in names)


def black_scholes_option_value(forward, volatility, maturity, strike, payoff_unit=1.0):
    """payoff_unit · (F·Φ(d₊) − K·Φ(d₋)): AnalyticFormulas.blackScholesGeneralizedOptionValue per path."""
    return option_formula("black_scholes", forward, volatility, maturity, strike, payoff_unit, ("value",))[0]


def bachelier_option_value(forward, volatility, maturity, strike, payoff_unit=1.0):
    """payoff_unit · ((F − K)·Φ(d) + σ√T·φ(d)), d = (F − K)/(σ√T): AnalyticFormulas.bachelierOptionValue per path."""
    return option_formula("bachelier", forward, volatility, maturity, strike, payoff_unit, ("value",))[0]


# ---------------------------------------------------------------- the implied volatility
IMPLIED_OUTPUTS = {"volatility": 1, "d_price": 2, "d_forward": 4}


def _implied_mask(outputs):
    if isinstance(outputs, str): outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or any(o not in IMPLIED_OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"implied_volatility: outputs {outputs!r} (distinct names out of {sorted(IMPLIED_OUTPUTS)})")
    return outputs, sum(IMPLIED_OUTPUTS[o] for o in outputs), [o for o in ("volatility", "d_price", "d_forward") if o in outputs]


def _time_value_double(m, F, s, K):
    """The time value of total volatility s from the out-of-the-money side, in double."""
    if m == 0:
        A, B = min(F, K), max(F, K)
        d = (math.log(A / B) + 0.5 * s * s) / s
        return A * _cdf(d) - B * _cdf(d - s)
    gap = abs(F - K)
    return s * _density(gap / s) - gap * _cdf(-gap / s)


def implied_volatility_double(model, price, forward, maturity, strike, payoff_unit=1.0) -> dict:
    """The implied volatility at doubles, in double: {"volatility", "d_price", "d_forward"} with the semantics of include/fmhip.h.  What a
    call with deterministic operands returns: a bisection on the time value in ln s, then Newton steps on the value."""
    m = _model(model)
    T, K = _check_scalars(maturity, strike)
    P, F, unit = float(price), float(forward), float(payoff_unit)
    nan = {"volatility": math.nan, "d_price": math.nan, "d_forward": math.nan}
    if any(v != v for v in (P, F, unit)) or not unit > 0.0: return nan
    c = P / unit
    if c != c: return nan
    intrinsic = max(F - K, 0.0)
    if c == intrinsic: return dict(nan, volatility=0.0)
    if not T > 0.0 or math.isinf(F) or c < intrinsic: return nan
    if m == 0:
        if not (F > 0.0 and K > 0.0) or c > F: return nan
        if c == F: return dict(nan, volatility=math.inf)
    elif math.isinf(c): return dict(nan, volatility=math.inf)
    tv = c - intrinsic
    lo, hi = -80.0, 80.0                                                      # ln s
    scale = 0.0 if m == 0 else math.log(max(abs(F - K), tv, 5e-324))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _time_value_double(m, F, math.exp(mid + scale), K) < tv: lo = mid
        else: hi = mid
    s = math.exp(0.5 * (lo + hi) + scale)
    for _ in range(3):
        slope = _density((math.log(min(F, K) / max(F, K)) + 0.5 * s * s) / s) * min(F, K) if m == 0 else _density(abs(F - K) / s)
        if not slope > 0.0: break
        step = (_time_value_double(m, F, s, K) - tv) / slope
        if not abs(step) < 0.5 * s: break
        s -= step
    sigma = s / math.sqrt(T)
    at = option_formula_double(model, F, sigma, T, K, 1.0)
    if sigma == 0.0 or math.isinf(sigma) or not at["vega"] > 0.0: return dict(nan, volatility=sigma)
    return {"volatility": sigma, "d_price": 1.0 / (unit * at["vega"]), "d_forward": -at["delta"] / at["vega"]}


def _implied_call(m, host, scalars, n, T, K, mask, n_out):
    out = [np.empty(n, dtype=np.float32) for _ in range(n_out)]
    cols = (C.c_void_p * n_out)(*[o.ctypes.data for o in out])
    ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in host]
    N.check(N.lib().fmhip_implied_volatility_host(m, ptr[0], scalars[0], ptr[1], scalars[1], ptr[2], scalars[2], n, T, K, mask, cols))
    return out


def implied_volatility_host(model, price, forward, maturity, strike, payoff_unit=1.0, outputs=("volatility",)) -> list:
    """The DEFINITION (fmhip_implied_volatility_host) over host arrays: price, forward and payoff_unit are float32 arrays of one size or
    numbers (fp64 scalars), at least one an array; one float32 array per name of `outputs`, in the order given."""
    m = _model(model)
    T, K = _check_scalars(maturity, strike)
    names, mask, in_bit_order = _implied_mask(outputs)
    arrays, scalars, n = [], [], None
    for o in (price, forward, payoff_unit):
        if np.isscalar(o):
            arrays.append(None); scalars.append(float(o))
        else:
            a = np.ascontiguousarray(o, dtype=np.float32).ravel()
            if n is not None and a.size != n: raise ValueError("implied_volatility: arrays of different size")
            n = a.size
            arrays.append(a); scalars.append(0.0)
    if n is None: raise ValueError("implied_volatility_host: at least one operand is an array (implied_volatility_double takes numbers)")
    by_name = dict(zip(in_bit_order, _implied_call(m, arrays, scalars, n, T, K, mask, len(in_bit_order))))
    return [by_name[o] for o in names]


def _implied_vectors(m, operands, T, K, mask, n_out):
    """fmhip_implied_volatility on DeviceVectors and floats: n_out new DeviceVectors, in bit order."""
    handles = [o.handle if isinstance(o, DeviceVector) else 0 for o in operands]
    scalars = [0.0 if isinstance(o, DeviceVector) else float(o) for o in operands]
    n = next(o.n for o in operands if isinstance(o, DeviceVector))
    if not device_analytic():
        host = [o.to_float32() if isinstance(o, DeviceVector) else None for o in operands]
        return [DeviceVector.from_host(o) for o in _implied_call(m, host, scalars, n, T, K, mask, n_out)]
    out = (C.c_int64 * n_out)()
    N.check(N.lib().fmhip_implied_volatility(m, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], T, K, mask, out))
    return [DeviceVector(int(h), n) for h in out]


def _inner_implied(model, operands, T, K, names, inner_factory=None):
    """The inverse on plain (not differentiable) operands — RandomVariableHip, numbers, or with inner_factory any RandomVariable with
    getRealizations: {name: RandomVariable} with the maximum filtration time."""
    m = _model(model)
    _, mask, in_bit_order = _implied_mask(names)
    times = [o.getFiltrationTime() for o in operands if not np.isscalar(o)]
    time = max(times) if times else -math.inf
    make = (lambda value: RandomVariableHip(time, value)) if inner_factory is None else (lambda value: inner_factory.createRandomVariable(time, value))
    if all(np.isscalar(o) or o.isDeterministic() for o in operands):
        P, F, unit = (float(o) if np.isscalar(o) else o.doubleValue() for o in operands)
        values = implied_volatility_double(model, P, F, T, K, unit)
        return {o: make(values[o]) for o in in_bit_order}
    if inner_factory is None:
        for o in operands:
            if not np.isscalar(o) and not isinstance(o, RandomVariableHip): raise TypeError(f"implied_volatility: {type(o).__name__} operands need the factory that made them (an AAD wrapper carries it)")
        plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else o.realizations for o in operands]
        return {o: make(v) for o, v in zip(in_bit_order, _implied_vectors(m, plain, T, K, mask, len(in_bit_order)))}
    plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else np.asarray(o.getRealizations(), dtype=np.float32) for o in operands]
    return {o: make(v) for o, v in zip(in_bit_order, implied_volatility_host(model, plain[0], plain[1], T, K, plain[2], in_bit_order))}


def _scaled(x, y, op):
    """x op y for numbers and RandomVariables on either side (op: "mult", "div", "add", "sub")."""
    if np.isscalar(x) and np.isscalar(y):
        return {"mult": x * y, "div": x / y, "add": x + y, "sub": x - y}[op]
    if np.isscalar(x):
        return {"mult": lambda: y.mult(x), "div": lambda: y.vid(x), "add": lambda: y.add(x), "sub": lambda: y.bus(x)}[op]()
    return getattr(x, op)(y)


def implied_volatility(model, price, forward, maturity, strike, payoff_unit=1.0, outputs=("volatility",), put=False):
    """The volatility per path at which fm.option_formula(model, forward, ·, maturity, strike, payoff_unit) has the value `price`, with —
    by name in `outputs` — "d_price" = ∂σ/∂price = 1/vega and "d_forward" = ∂σ/∂forward = −delta/vega at the root: price, forward and
    payoff_unit are RandomVariableHip or numbers, maturity >= 0 is a number, strike a number or a RandomVariable.  One launch whatever the
    outputs; operands stay where they are.  Returns one RandomVariable per name, as a tuple in the order given; the filtration time is
    the operands' maximum.  Deterministic operands give a deterministic result computed in double.  A price at the intrinsic value gives
    volatility 0, a Black–Scholes price equal to the forward +∞ (partials NaN); a price outside the no-arbitrage bounds, a payoff unit
    <= 0, maturity 0 with a time value, and a NaN give NaN (include/fmhip.h has the list).

    put=True: `price` is a put's; it is converted by parity, price + payoff_unit·(forward − strike), before the call, and "d_forward"
    is the put's.  A strike that is a RandomVariable is normalised away — Black–Scholes: price/K, forward/K, strike 1; Bachelier:
    forward − K, strike 0 — the entry point keeps a scalar strike; the partials are those in the operands given.

    RandomVariableDifferentiableAAD operands: ONE launch with payoff unit 1 and all three outputs on c = price/payoff_unit; the partials in
    c and the forward are recorded, and ∂σ/∂payoff_unit = −(price/payoff_unit)·∂σ/∂price follows from the recorded division.  A "d_price" or
    "d_forward" asked for by name is, as without AAD, the partial in the operand given (a put's, with a strike per path), itself not
    differentiable further."""
    from .differentiable import RandomVariableDifferentiableAAD, _Node
    names, _, _ = _implied_mask(outputs)
    T, _ = _check_scalars(maturity, 0.0)
    m = _model(model)
    given_forward, K_vector = forward, None
    if put: price = _scaled(price, _scaled(payoff_unit, _scaled(forward, strike, "sub"), "mult"), "add")
    if not np.isscalar(strike):
        if strike.isDeterministic(): strike = strike.doubleValue()
        elif m == 0: K_vector, price, forward, strike = strike, _scaled(price, strike, "div"), _scaled(forward, strike, "div"), 1.0
        else: forward, strike = _scaled(forward, strike, "sub"), 0.0
    _, K = _check_scalars(maturity, strike)
    operands = (price, forward, payoff_unit)
    if not any(isinstance(o, RandomVariableDifferentiableAAD) for o in operands):
        wanted = set(names) | ({"d_price"} if put and "d_forward" in names else set())
        results = _inner_implied(model, operands, T, K, tuple(o for o in ("volatility", "d_price", "d_forward") if o in wanted))
        if K_vector is not None:                                                   # ∂/∂(price/K) and ∂/∂(forward/K) to ∂/∂price and ∂/∂forward
            for name in ("d_price", "d_forward"):
                if name in results: results[name] = results[name].div(K_vector)
        if put and "d_forward" in results: results["d_forward"] = results["d_forward"].add(_scaled(results["d_price"], payoff_unit, "mult"))
        return tuple(results[o] for o in names)
    factory = next(o.factory for o in operands if isinstance(o, RandomVariableDifferentiableAAD))
    c = price if np.isscalar(payoff_unit) and float(payoff_unit) == 1.0 else _scaled(price, payoff_unit, "div")
    ops = (c, forward)
    inner = [o.values if isinstance(o, RandomVariableDifferentiableAAD) else o for o in ops]
    hip = all(np.isscalar(o) or isinstance(o, RandomVariableHip) for o in inner)
    if not hip and factory is None: raise NotImplementedError("implied_volatility on this inner implementation needs the factory that made the variables")
    unit = _inner_implied(model, (inner[0], inner[1], 1.0), T, K, ("volatility", "d_price", "d_forward"), None if hip else factory.inner)
    nodes = tuple(o.node if isinstance(o, RandomVariableDifferentiableAAD) else None for o in ops)
    sigma = RandomVariableDifferentiableAAD(unit["volatility"], _Node("IMPLIED_VOLATILITY", nodes, (unit["d_price"], unit["d_forward"]), 0.0), factory)
    results = {"volatility": sigma}
    if "d_price" in names or "d_forward" in names:
        # the partials asked for by name: those of the plain branch, in the operands GIVEN — from ∂/∂c and ∂/∂(the forward handed to the entry
        # point) by the chain rule on the inner values; not differentiable further
        plain = lambda o: o.values if isinstance(o, RandomVariableDifferentiableAAD) else o
        d_price, d_forward = unit["d_price"], unit["d_forward"]
        if not (np.isscalar(payoff_unit) and float(payoff_unit) == 1.0): d_price = _scaled(d_price, plain(payoff_unit), "div")      # c = price/N
        if K_vector is not None: d_price, d_forward = _scaled(d_price, plain(K_vector), "div"), _scaled(d_forward, plain(K_vector), "div")
        if put: d_forward = _scaled(d_forward, _scaled(d_price, plain(payoff_unit), "mult"), "add")
        for name, value in (("d_price", d_price), ("d_forward", d_forward)):
            if name in names: results[name] = RandomVariableDifferentiableAAD(value, None, factory)
    return tuple(results[o] for o in names)


def black_scholes_implied_volatility(price, forward, maturity, strike, payoff_unit=1.0, put=False):
    """The σ with payoff_unit · (F·Φ(d₊) − K·Φ(d₋)) = price, per path: AnalyticFormulas.blackScholesOptionImpliedVolatility."""
    return implied_volatility("black_scholes", price, forward, maturity, strike, payoff_unit, ("volatility",), put)[0]


def bachelier_implied_volatility(price, forward, maturity, strike, payoff_unit=1.0, put=False):
    """The σ with payoff_unit · ((F − K)·Φ(d) + σ√T·φ(d)) = price, per path: AnalyticFormulas.bachelierOptionImpliedVolatility."""
    return implied_volatility("bachelier", price, forward, maturity, strike, payoff_unit, ("volatility",), put)[0]


def convert_volatility(from_model, to_model, forward, volatility, maturity, strike):
    """The volatility of `to_model` that gives the price `from_model` gives with `volatility` (lognormal to normal, or back), per path:
    one option_formula followed by one implied_volatility — two launches."""
    value, = option_formula(from_model, forward, volatility, maturity, strike, 1.0, ("value",))
    return implied_volatility(to_model, value, forward, maturity, strike, 1.0, ("volatility",))[0]
