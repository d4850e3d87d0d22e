"""Transform option values per path on the device (include/fmhip.h: fmhip_transform_option and its _host twin; host/transform_formula.hpp;
DESIGN.md §4.28): the value of a call, with its partials in the forward and in the first state, under a model whose characteristic function
is exponential-affine in at most two state variables — Black–Scholes and Merton (no state), Heston and Bates (the variance) — given the state
of every path, on vectors that already live in HBM: the forward smile, exposures of options under stochastic volatility, model prices as
control variates, without an inner simulation.

THE FORMULA.  With x = ln(S_T/F) and E exp(izx) = exp(C(z) + Σ_s D_s(z)·V_s), Lewis' single integral for the call in forward form is
    value = N·(F − √(FK)/π · ∫₀^∞ Re[exp(iuk)·φ(u − i/2)] / (u² + ¼) du),      k = ln(F/K)
and a fixed quadrature (u_j, w_j) leaves a finite sum of exp(real affine in the states)·cos(real affine in the states and k): the NODE TABLE
holds, per node, u_j, a = C(u_j − i/2) + ln(w_j/(π(u_j² + ¼))) and b_s = D_s(u_j − i/2), as real and imaginary parts.  C and D are computed
here once, in numpy complex128; the device's work per element is J × (one exp, one sine/cosine pair, a handful of products).

C AND D OF HESTON use the formulation that needs no branch tracking of the complex logarithm (Albrecher, Mayer, Schoutens, Tistaert 2007):
    β = κ − iρξz,   d = √(β² + ξ²(z² + iz)),   g = (β − d)/(β + d),
    D = (β − d)/ξ² · (1 − e^{−dT})/(1 − g e^{−dT}),   C = κθ/ξ² · ((β − d)T − 2 ln((1 − g e^{−dT})/(1 − g)))
Bates adds Merton's jump term λT(exp(izμ − δ²z²/2) − 1 − iz(e^{μ+δ²/2} − 1)) to C.

THE RULE is Gauss–Legendre in x on [0, 1] after the substitution u = u_max·x²: the integrand is even in u, so it stays analytic in x; the
nodes crowd at u = 0, where 1/(u² + ¼) peaks (its width is ½ whatever the model), as (j/J)²·u_max, and thin out to 2·u_max/J at the far end,
where only the oscillation exp(iuk) is left to resolve.  u_max is the first point of a geometric grid from which the integrand's envelope
|φ(u − i/2)|/(π·u) stays below tolerance/8 at every probe state.  With n_nodes=None the number of nodes doubles from 32 until the
definition's values before narrowing at the probe states (every probe state × every probe moneyness, F = 1) change by less than the tolerance from J to 2J
nodes; the table of 2J nodes is returned, with that change as `measured`.  256 nodes that do not get there raise ValueError: no table is
returned that is silently wrong.  The default tolerance is 2⁻²⁴ (relative to the forward): the output is fp32 and a price never exceeds F.

FMHIP_DEVICE_ANALYTIC=0, read per call: the A/B switch and the fallback — the vectors are downloaded, the definition runs on one core, and
the results are uploaded.  The device path never falls back on its own: a missing kernel is an error.
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np

from . import _native as N
from .analytic import _scaled, device_analytic
from .random_variable import DeviceVector, RandomVariableHip

OUTPUTS = {"value": 1, "delta": 2, "state_delta": 4}
MAX_NODES = 256
MAX_STATES = 2
DEFAULT_TOLERANCE = 2.0 ** -24
DEFAULT_PROBE_MONEYNESS = (0.5, 1.0, 2.0)                                    # F/K

_pd = C.POINTER(C.c_double)


class TransformNodes:
    """A node table of fmhip_transform_option: `table` (J rows of 3 + 2·n_states doubles: u, a_re, a_im, b_re[], b_im[]), `n_states`, the
    `rule` that made it, the `tolerance` it was asked to meet (relative to the forward) and the change `measured` at the probe states
    between half its nodes and all of them (None for a table of a given size)."""

    def __init__(self, table, n_states, rule="given", tolerance=None, measured=None, u_max=None):
        table = np.ascontiguousarray(table, dtype=np.float64)
        n_states = int(n_states)
        if not 0 <= n_states <= MAX_STATES: raise ValueError(f"transform nodes: {n_states} state variables (0 … {MAX_STATES})")
        if table.ndim != 2 or table.shape[1] != 3 + 2 * n_states or not 1 <= table.shape[0] <= MAX_NODES:
            raise ValueError(f"transform nodes: a table of 1 … {MAX_NODES} rows of {3 + 2 * n_states} doubles")
        if not np.isfinite(table).all(): raise ValueError("transform nodes: an entry of the table is not finite")
        self.table, self.n_states, self.rule, self.tolerance, self.measured, self.u_max = table, n_states, rule, tolerance, measured, u_max

    @property
    def n_nodes(self): return self.table.shape[0]

    def __repr__(self):
        return f"TransformNodes({self.n_nodes} nodes, {self.n_states} states, rule={self.rule!r}, tolerance={self.tolerance}, measured={self.measured})"


# ---------------------------------------------------------------- the models: (C, [D_s]) at z = u − i/2, in complex128
def _black_scholes_exponent(total_variance):
    return lambda z: (-0.5 * total_variance * (z * z + 1j * z), [])


def _jump_term(jump_intensity, jump_size_mean, jump_size_stddev, maturity, z):
    m = math.exp(jump_size_mean + 0.5 * jump_size_stddev * jump_size_stddev)
    return jump_intensity * maturity * (np.exp(1j * z * jump_size_mean - 0.5 * jump_size_stddev * jump_size_stddev * z * z) - 1.0 - 1j * z * (m - 1.0))


def _heston_exponent(kappa, theta, xi, rho, maturity):
    def exponent(z):
        beta = kappa - 1j * rho * xi * z
        d = np.sqrt(beta * beta + xi * xi * (z * z + 1j * z))
        g = (beta - d) / (beta + d)
        decay = np.exp(-d * maturity)
        D = (beta - d) / (xi * xi) * (1.0 - decay) / (1.0 - g * decay)
        Cz = kappa * theta / (xi * xi) * ((beta - d) * maturity - 2.0 * np.log((1.0 - g * decay) / (1.0 - g)))
        return Cz, [D]
    return exponent


def _plus(exponent, extra):
    def both(z):
        Cz, D = exponent(z)
        return Cz + extra(z), D
    return both


# ---------------------------------------------------------------- the rule
@functools.lru_cache(maxsize=None)
def _gauss_legendre(n_nodes):
    """Nodes and weights on [0, 1]; kept: numpy finds them as eigenvalues, a millisecond at 256, and a driver asks again per call."""
    x, w = np.polynomial.legendre.leggauss(n_nodes)
    x, w = 0.5 * (x + 1.0), 0.5 * w
    x.setflags(write=False); w.setflags(write=False)
    return x, w


def _table(exponent, n_states, n_nodes, u_max):
    x, w = _gauss_legendre(int(n_nodes))
    u = u_max * x * x
    weight = w * 2.0 * u_max * x                                              # du = 2·u_max·x dx
    Cz, D = exponent(u - 0.5j)
    Cz = np.broadcast_to(np.asarray(Cz, dtype=np.complex128), u.shape)
    table = np.empty((u.size, 3 + 2 * n_states), dtype=np.float64)
    table[:, 0] = u
    table[:, 1] = Cz.real + np.log(weight / (math.pi * (u * u + 0.25)))
    table[:, 2] = Cz.imag
    for s in range(n_states):
        table[:, 3 + s] = D[s].real
        table[:, 3 + n_states + s] = D[s].imag
    return table


def _u_max(exponent, probe_states, tolerance):
    """The first point of a geometric grid from which |φ(u − i/2)|/(π u) is below tolerance/8 at every probe state, at it and beyond."""
    grid = 2.0 ** (np.arange(0, 15 * 8 + 1) / 8.0)                            # 1 … 2^15
    Cz, D = exponent(grid - 0.5j)
    exponent_re = np.broadcast_to(np.asarray(Cz, dtype=np.complex128).real, grid.shape)
    worst = np.full(grid.shape, -np.inf)
    for state in probe_states:
        e = exponent_re.copy()
        for s, v in enumerate(state): e = e + D[s].real * v
        worst = np.maximum(worst, e)
    envelope = np.exp(worst) / (math.pi * grid)
    beyond = np.maximum.accumulate(envelope[::-1])[::-1]
    ok = np.nonzero(beyond <= tolerance / 8.0)[0]
    if ok.size == 0: raise ValueError("transform nodes: the integrand does not fall below the tolerance before u = 2^15 at a probe state")
    return float(grid[ok[0]])


def _probe_values(table, n_states, probe_states, probe_moneyness):
    """The definition's value at F = 1, K = 1/m for every probe state × moneyness, BEFORE it is narrowed: the same finite sum over the table,
    taken in numpy in fp64 (the entry point's fp32 result carries 2⁻²⁵ of rounding, the size of what is compared here)."""
    out = []
    for state in probe_states:
        for m in probe_moneyness:
            k = math.log(float(m))
            e = table[:, 1].copy(); th = table[:, 2] + table[:, 0] * k
            for s, v in enumerate(state):
                e = e + table[:, 3 + s] * v
                th = th + table[:, 3 + n_states + s] * v
            out.append(1.0 - math.sqrt(1.0 / float(m)) * float(np.sum(np.exp(e) * np.cos(th))))
    return np.array(out)


def _build(exponent, n_states, probe_states, probe_moneyness, n_nodes, tolerance, rule):
    tolerance = float(tolerance)
    if not tolerance > 0.0: raise ValueError("transform nodes: the tolerance is positive")
    probe_states = [tuple(float(v) for v in (s if np.ndim(s) else (s,)))[:n_states] for s in probe_states] if n_states else [()]
    u_max = _u_max(exponent, probe_states, tolerance)
    if n_nodes is not None:
        n_nodes = int(n_nodes)
        if not 1 <= n_nodes <= MAX_NODES: raise ValueError(f"transform nodes: {n_nodes} nodes (1 … {MAX_NODES})")
        return TransformNodes(_table(exponent, n_states, n_nodes, u_max), n_states, rule, tolerance, None, u_max)
    J = 32
    previous = _probe_values(_table(exponent, n_states, J, u_max), n_states, probe_states, probe_moneyness)
    while 2 * J <= MAX_NODES:
        J *= 2
        table = _table(exponent, n_states, J, u_max)
        values = _probe_values(table, n_states, probe_states, probe_moneyness)
        change = float(np.max(np.abs(values - previous)))
        if change < tolerance: return TransformNodes(table, n_states, rule, tolerance, change, u_max)
        previous = values
    raise ValueError(f"transform nodes: {MAX_NODES} nodes leave a change of {change:.3g} at the probe states, above the tolerance {tolerance:.3g} "
                     f"(u_max = {u_max:.4g}): a short maturity at a vanishing variance needs more than this rule has")


RULE = "Gauss-Legendre in x, u = u_max x^2"


def black_scholes_transform_nodes(volatility, maturity, n_nodes=None, tolerance=DEFAULT_TOLERANCE, probe_moneyness=DEFAULT_PROBE_MONEYNESS):
    """The nodes of a Black–Scholes call with the volatility σ and the maturity T: no state; fm.option_formula's value by another road."""
    w = float(volatility) ** 2 * float(maturity)
    if not (w > 0.0 and math.isfinite(w)): raise ValueError("transform nodes: σ²T is positive and finite")
    return _build(_black_scholes_exponent(w), 0, [()], probe_moneyness, n_nodes, tolerance, RULE)


def merton_transform_nodes(volatility, jump_intensity, jump_size_mean, jump_size_stddev, maturity, n_nodes=None, tolerance=DEFAULT_TOLERANCE,
                           probe_moneyness=DEFAULT_PROBE_MONEYNESS):
    """The nodes of Merton's jump diffusion (montecarlo.merton_call_mc's parameters): no state."""
    T = float(maturity)
    w = float(volatility) ** 2 * T
    if not (w > 0.0 and math.isfinite(w)): raise ValueError("transform nodes: σ²T is positive and finite")
    jump = lambda z: _jump_term(float(jump_intensity), float(jump_size_mean), float(jump_size_stddev), T, z)
    return _build(_plus(_black_scholes_exponent(w), jump), 0, [()], probe_moneyness, n_nodes, tolerance, RULE)


def _heston_checked(kappa, theta, xi, rho, maturity):
    kappa, theta, xi, rho, T = float(kappa), float(theta), float(xi), float(rho), float(maturity)
    if not (kappa > 0.0 and theta > 0.0 and xi > 0.0 and -1.0 < rho < 1.0 and T > 0.0 and all(math.isfinite(v) for v in (kappa, theta, xi, T))):
        raise ValueError("transform nodes: Heston needs κ, θ, ξ, T > 0 and |ρ| < 1")
    return kappa, theta, xi, rho, T


def heston_transform_nodes(kappa, theta, xi, rho, maturity, n_nodes=None, tolerance=DEFAULT_TOLERANCE, probe_variances=None,
                           probe_moneyness=DEFAULT_PROBE_MONEYNESS):
    """The nodes of Heston's model for the maturity T: one state, the variance v_t of the path.  probe_variances: the variances at which the
    number of nodes is judged — the default is (1e-4, θ, max(0.3, 4θ)): the smallest decides how far the integrand reaches, the largest
    how fast it turns."""
    kappa, theta, xi, rho, T = _heston_checked(kappa, theta, xi, rho, maturity)
    if probe_variances is None: probe_variances = (1e-4, theta, max(0.3, 4.0 * theta))
    return _build(_heston_exponent(kappa, theta, xi, rho, T), 1, list(probe_variances), probe_moneyness, n_nodes, tolerance, RULE)


def bates_transform_nodes(kappa, theta, xi, rho, jump_intensity, jump_size_mean, jump_size_stddev, maturity, n_nodes=None, tolerance=DEFAULT_TOLERANCE,
                          probe_variances=None, probe_moneyness=DEFAULT_PROBE_MONEYNESS):
    """The nodes of Bates' model: Heston's variance and Merton's jumps; one state.  With jump_intensity 0 the table is Heston's, bit for bit."""
    kappa, theta, xi, rho, T = _heston_checked(kappa, theta, xi, rho, maturity)
    if probe_variances is None: probe_variances = (1e-4, theta, max(0.3, 4.0 * theta))
    jump = lambda z: _jump_term(float(jump_intensity), float(jump_size_mean), float(jump_size_stddev), T, z)
    return _build(_plus(_heston_exponent(kappa, theta, xi, rho, T), jump), 1, list(probe_variances), probe_moneyness, n_nodes, tolerance, RULE)


# ---------------------------------------------------------------- the pass
def _mask(outputs, n_states):
    if isinstance(outputs, str): outputs = (outputs,)
    outputs = tuple(outputs)
    if not outputs or any(o not in OUTPUTS for o in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"transform_option: outputs {outputs!r} (distinct names out of {sorted(OUTPUTS)})")
    if "state_delta" in outputs and n_states == 0: raise ValueError("transform_option: the state delta needs a state variable")
    return outputs, sum(OUTPUTS[o] for o in outputs), [o for o in ("value", "delta", "state_delta") if o in outputs]


def _states(nodes, states):
    if states is None: states = ()
    if np.isscalar(states) or not isinstance(states, (tuple, list)): states = (states,)
    if len(states) != nodes.n_states: raise ValueError(f"transform_option: {len(states)} states for nodes of {nodes.n_states}")
    return tuple(states)


def _host_call(nodes, arrays, scalars, n, K, mask, n_out):
    """fmhip_transform_option_host; arrays and scalars in the order forward, payoff unit, the states."""
    out = [np.empty(n, dtype=np.float32) for _ in range(n_out)]
    cols = (C.c_void_p * n_out)(*[o.ctypes.data for o in out])
    ptr = [a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays]
    S = nodes.n_states
    state_ptrs = (C.c_void_p * max(S, 1))(*[ptr[2 + s] for s in range(S)]) if S else None
    state_scalars = (C.c_double * max(S, 1))(*[scalars[2 + s] for s in range(S)]) if S else None
    N.check(N.lib().fmhip_transform_option_host(nodes.table.ctypes.data_as(_pd), nodes.n_nodes, S, ptr[0], scalars[0], state_ptrs, state_scalars, ptr[1], scalars[1],
                                                n, K, mask, cols))
    return out


def transform_option_host(nodes, forward, states, strike, payoff_unit=1.0, outputs=("value",)) -> list:
    """The DEFINITION (fmhip_transform_option_host) over host arrays: forward, payoff_unit and every state are float32 arrays of one size or
    numbers (fp64 scalars), at least one an array; one float32 array per name of `outputs`, in the order given."""
    states = _states(nodes, states)
    names, mask, in_bit_order = _mask(outputs, nodes.n_states)
    K = float(strike)
    if K != K: raise ValueError("transform_option: the strike is a NaN")
    arrays, scalars, n = [], [], None
    for o in (forward, payoff_unit) + states:
        if np.isscalar(o):
            arrays.append(None); scalars.append(float(o))
        else:
            a = np.ascontiguousarray(o, dtype=np.float32).ravel()
            if n is not None and a.size != n: raise ValueError("transform_option: arrays of different size")
            n = a.size
            arrays.append(a); scalars.append(0.0)
    if n is None: raise ValueError("transform_option_host: at least one operand is an array")
    by_name = dict(zip(in_bit_order, _host_call(nodes, arrays, scalars, n, K, mask, len(in_bit_order))))
    return [by_name[o] for o in names]


def _vectors(nodes, operands, K, mask, n_out):
    """fmhip_transform_option on DeviceVectors and floats (forward, payoff unit, the states): n_out new DeviceVectors, in bit order."""
    handles = [o.handle if isinstance(o, DeviceVector) else 0 for o in operands]
    scalars = [0.0 if isinstance(o, DeviceVector) else float(o) for o in operands]
    n = next(o.n for o in operands if isinstance(o, DeviceVector))
    if not device_analytic():
        host = [o.to_float32() if isinstance(o, DeviceVector) else None for o in operands]
        return [DeviceVector.from_host(o) for o in _host_call(nodes, host, scalars, n, K, mask, n_out)]
    S = nodes.n_states
    state_handles = (C.c_int64 * max(S, 1))(*[handles[2 + s] for s in range(S)]) if S else None
    state_scalars = (C.c_double * max(S, 1))(*[scalars[2 + s] for s in range(S)]) if S else None
    out = (C.c_int64 * n_out)()
    N.check(N.lib().fmhip_transform_option(nodes.table.ctypes.data_as(_pd), nodes.n_nodes, S, handles[0], scalars[0], state_handles, state_scalars, handles[1], scalars[1],
                                           K, mask, out))
    return [DeviceVector(int(h), n) for h in out]


def _inner(nodes, operands, K, names, inner_factory=None):
    """The pass on plain (not differentiable) operands (forward, payoff unit, the states) — RandomVariableHip, numbers, or with inner_factory
    any RandomVariable with getRealizations: {name: RandomVariable} with the maximum filtration time.  Deterministic operands go through the
    host twin with the payoff unit as a vector of one element: the result is the definition's, narrowed to fp32."""
    _, mask, in_bit_order = _mask(names, nodes.n_states)
    times = [o.getFiltrationTime() for o in operands if not np.isscalar(o)]
    time = max(times) if times else -math.inf
    make = (lambda value: RandomVariableHip(time, value)) if inner_factory is None else (lambda value: inner_factory.createRandomVariable(time, value))
    if all(np.isscalar(o) or o.isDeterministic() for o in operands):
        flat = [float(o) if np.isscalar(o) else o.doubleValue() for o in operands]
        unit = transform_option_host(nodes, flat[0], tuple(flat[2:]), K, np.ones(1, dtype=np.float32), in_bit_order)
        return {o: make(float(v[0]) * flat[1]) for o, v in zip(in_bit_order, unit)}
    if inner_factory is None:
        for o in operands:
            if not np.isscalar(o) and not isinstance(o, RandomVariableHip): raise TypeError(f"transform_option: {type(o).__name__} operands need the factory that made them (an AAD wrapper carries it)")
        plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else o.realizations for o in operands]
        return {o: make(v) for o, v in zip(in_bit_order, _vectors(nodes, plain, K, mask, len(in_bit_order)))}
    plain = [float(o) if np.isscalar(o) else o.doubleValue() if o.isDeterministic() else np.asarray(o.getRealizations(), dtype=np.float32) for o in operands]
    return {o: make(v) for o, v in zip(in_bit_order, transform_option_host(nodes, plain[0], tuple(plain[2:]), K, plain[1], in_bit_order))}


def transform_option_value(nodes, forward, states, strike, payoff_unit=1.0, outputs=("value",), put=False):
    """Value, delta (∂/∂forward) and state delta (∂/∂ the first state) of a CALL in forward form under the model of `nodes` (a
    TransformNodes), per path: forward, payoff_unit (a discount factor, a notional) and the states (a tuple of nodes.n_states; one state may
    be given bare) are RandomVariableHip or numbers, strike a number or a RandomVariable.  One launch whatever the outputs; operands stay
    where they are.  Returns one RandomVariable per name of `outputs`, as a tuple in the order given; the filtration time is the operands'
    maximum.  An element with forward <= 0 or strike <= 0 is the limit: intrinsic value, a step delta, state delta 0.  Nothing is clamped to
    the arbitrage bounds.

    put=True: by parity, the call minus payoff_unit·(forward − strike); the delta minus payoff_unit.  A strike that is a RandomVariable is
    normalised away by homogeneity — forward/K at the strike 1, value and state delta times K — the entry point keeps a scalar strike.

    RandomVariableDifferentiableAAD operands: ONE launch with payoff unit 1 and every output the model has; value·payoff_unit is formed with
    the recorded operations, and delta and state delta are the recorded partials in the forward and the first state.  A "delta" or
    "state_delta" asked for by name is payoff_unit times that vector, itself not differentiable further."""
    from .differentiable import RandomVariableDifferentiableAAD, _Node
    states = _states(nodes, states)
    names, _, _ = _mask(outputs, nodes.n_states)
    given_forward, K_vector = forward, None
    if not np.isscalar(strike):
        if strike.isDeterministic(): strike = strike.doubleValue()
        else: K_vector, forward, strike = strike, _scaled(forward, strike, "div"), 1.0
    K = float(strike)
    if K != K: raise ValueError("transform_option: the strike is a NaN")
    operands = (forward, payoff_unit) + states
    if not any(isinstance(o, RandomVariableDifferentiableAAD) for o in operands):
        results = _inner(nodes, operands, K, names)
    else:
        if nodes.n_states == 2 and isinstance(states[1], RandomVariableDifferentiableAAD):
            raise NotImplementedError("transform_option: the pass has the partial in the first state only; the second state cannot be differentiable")
        factory = next(o.factory for o in operands if isinstance(o, RandomVariableDifferentiableAAD))
        inner = [o.values if isinstance(o, RandomVariableDifferentiableAAD) else o for o in operands]
        hip = all(np.isscalar(o) or isinstance(o, RandomVariableHip) for o in inner)
        if not hip and factory is None: raise NotImplementedError("transform_option on this inner implementation needs the factory that made the variables")
        every = ("value", "delta") + (("state_delta",) if nodes.n_states else ())
        unit = _inner(nodes, (inner[0], 1.0) + tuple(inner[2:]), K, every, None if hip else factory.inner)
        differentiable = (forward,) + states[:1]
        arg_nodes = tuple(o.node if isinstance(o, RandomVariableDifferentiableAAD) else None for o in differentiable)
        value = RandomVariableDifferentiableAAD(unit["value"], _Node("TRANSFORM_OPTION", arg_nodes, tuple(unit[o] for o in every[1:]), 0.0), factory)
        results = {"value": value if np.isscalar(payoff_unit) and float(payoff_unit) == 1.0 else value.mult(payoff_unit)}
        for name in ("delta", "state_delta"):
            if name in names: results[name] = RandomVariableDifferentiableAAD(_scaled(unit[name], inner[1], "mult"), None, factory)
    if K_vector is not None:                                                   # K·f(F/K, 1): the value and ∂/∂V scale with K, ∂/∂F does not
        for name in ("value", "state_delta"):
            if name in results: results[name] = results[name].mult(K_vector)
        strike = K_vector
    if put:
        if "value" in results: results["value"] = results["value"].sub(_scaled(payoff_unit, _scaled(given_forward, strike, "sub"), "mult"))
        if "delta" in results: results["delta"] = results["delta"].sub(payoff_unit)
    return tuple(results[o] for o in names)


def heston_option_value(forward, variance, maturity, strike, kappa, theta, xi, rho, payoff_unit=1.0, outputs=("value",), put=False, nodes=None, **node_arguments):
    """The Heston value per path of a call (put=True: a put) expiring `maturity` from now, given the forward and the variance of every path:
    transform_option_value on heston_transform_nodes(kappa, theta, xi, rho, maturity, **node_arguments), or on `nodes` where a caller keeps
    the table (it depends on the model and the maturity alone)."""
    if nodes is None: nodes = heston_transform_nodes(kappa, theta, xi, rho, maturity, **node_arguments)
    return transform_option_value(nodes, forward, (variance,), strike, payoff_unit, outputs, put)


def bates_option_value(forward, variance, maturity, strike, kappa, theta, xi, rho, jump_intensity, jump_size_mean, jump_size_stddev, payoff_unit=1.0,
                       outputs=("value",), put=False, nodes=None, **node_arguments):
    """heston_option_value with Merton's jumps in the price (bates_transform_nodes)."""
    if nodes is None: nodes = bates_transform_nodes(kappa, theta, xi, rho, jump_intensity, jump_size_mean, jump_size_stddev, maturity, **node_arguments)
    return transform_option_value(nodes, forward, (variance,), strike, payoff_unit, outputs, put)


def heston_call_analytic(initial_value, risk_free_rate, v0, kappa, theta, xi, rho, maturity, strike, **node_arguments):
    """The Heston call at a number, beside montecarlo.merton_call_analytic: the host definition on the forward S₀e^{rT} and the variance v0
    as fp64 scalars, discounted.  The definition narrows its result to fp32 once."""
    node_arguments.setdefault("probe_variances", (float(v0),))
    node_arguments.setdefault("probe_moneyness", (float(initial_value) * math.exp(risk_free_rate * maturity) / float(strike),))
    nodes = heston_transform_nodes(kappa, theta, xi, rho, maturity, **node_arguments)
    value, = transform_option_host(nodes, float(initial_value) * math.exp(risk_free_rate * maturity), (float(v0),), strike, np.ones(1, dtype=np.float32))
    return float(value[0]) * math.exp(-risk_free_rate * maturity)
