"""Small Monte-Carlo drivers written ONLY against the RandomVariable / BrownianMotion interfaces — the callers on
the other side of the hot path.  They accept any factory / Brownian motion that
implements the interface (RandomVariableHip…, or the CPU twin in the tests), exactly as finmath-lib's models accept
a RandomVariableFactory by injection (LIBORMarketModelCalibrationATMTest.java:351-358).

    black_scholes_call_mc   MonteCarloBlackScholesModelTest.java:62-85,125-157 (Euler scheme on the log state,
                            numeraire exp(r t), European call)
    local_volatility_call_mc  the same scheme under a tabulated surface σ(t, S): the volatility of a step is a row of the surface applied
                            to the state by RandomVariable.apply(TabulatedFunction) (tabulated.py)
    heston_call_mc          BASELINE.json configs[2]: Euler full-truncation Heston driven by BrownianMotionHip
    heston_call_conditional_mc  the same scheme by conditional Monte-Carlo: the variance path alone is simulated, the payoff's conditional
                            expectation is a Black–Scholes value per path (analytic.py)
    stochastic_local_volatility_call_mc  Heston's variance under a leverage function calibrated to a Dupire surface by the particle
                            method: E[v | ln S] re-estimated at every step by kernel regression on the device (kernel_regression.py,
                            DESIGN.md §4.19)
    geometric_asian_call_mc a call on the geometric average over the points of the time discretisation — a path-dependent product with a
                            closed form (geometric_asian_call_analytic), where a Brownian bridge over Sobol' points (sobol.py) has
                            something to show
    merton_call_mc          Merton's jump-diffusion driven by IndependentIncrementsFromICDF (increments.py: Brownian increment, normal
                            jump size, Poisson jump count), with merton_call_analytic, Merton's series, as its closed-form check
    merton_call_by_jump_count_mc  the same simulation with the payoff grouped by the number of jumps on the device (group.py, DESIGN.md
                            §4.29): Merton's series term by term
    variance_gamma_call_mc  the variance-gamma model (Madan, Carr, Chang 1998) driven by VarianceGammaProcess (increments.py: a gamma clock
                            and a standard normal per step), with variance_gamma_call_analytic — Black–Scholes conditional on the gamma
                            time, integrated against its density — as its check
    bermudan_option_mc      Longstaff–Schwartz backward induction over MonteCarloConditionalExpectationRegression (regression.py):
                            what finmath-lib's BermudanOption does with its conditional-expectation estimator
    bermudan_option_bounds_mc  the primal–dual bounds of Andersen & Broadie for the same option: the fitted policy on fresh paths, and a
                            martingale from inner simulations at every exercise date of every outer path (nested.py)
    nested_initial_margin_mc  the dynamic initial margin of a forward contract at a future date: the quantile, per outer state, of the inner
                            P&L over the margin period of risk — a block order statistic (nested.py)
    forward_implied_volatility_mc  the forward smile: the distribution, at a future date, of the volatility implied by a call's price under
                            heston_call_mc's scheme — inner means per outer state, inverted per path (analytic.py)
    particle_filter_log_likelihood  the bootstrap particle filter of a linear-Gaussian state-space model — propagate, weight by the
                            observation density, resample on the device (resample.py) — with kalman_log_likelihood, the
                            exact answer, as its check; stochastic_volatility_log_likelihood is the same filter on the discrete
                            stochastic-volatility model, which has no closed form
    bermudan_max_call_mc    the same induction for a call on the maximum of several assets, regressed on all monomials of the assets up
                            to a total degree: 10 … 56 basis functions, the wide one-pass normal equations
"""
from __future__ import annotations

import math


def black_scholes_call_mc(brownian_motion, initial_value, risk_free_rate, volatility, maturity, strike):
    """Value of a European call under Black–Scholes by Monte-Carlo: log-Euler scheme
    X_{i+1} = X_i + (r - σ²/2) Δt_i + σ ΔW_i, S = exp(X); payoff max(S_T - K, 0) / exp(r T).
    `maturity` must be a point of the Brownian motion's time discretisation."""
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw = brownian_motion.getBrownianIncrement(i, 0)
        x = x.add((risk_free_rate - 0.5 * volatility * volatility) * dt).addProduct(dw, volatility)
        i += 1
        t = td.getTime(i)
    payoff = x.exp().sub(strike).floor(0.0)
    value = payoff.div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value


def black_scholes_call_analytic(initial_value, risk_free_rate, volatility, maturity, strike):
    """net.finmath.functions.AnalyticFormulas.blackScholesOptionValue (closed form)."""
    from math import erf, exp, log, sqrt
    d1 = (log(initial_value / strike) + (risk_free_rate + 0.5 * volatility ** 2) * maturity) / (volatility * sqrt(maturity))
    d2 = d1 - volatility * sqrt(maturity)
    cdf = lambda z: 0.5 * (1.0 + erf(z / sqrt(2.0)))
    return initial_value * cdf(d1) - strike * exp(-risk_free_rate * maturity) * cdf(d2)


def local_volatility_call_mc(brownian_motion, initial_value, risk_free_rate, times, spots, vols, maturity, strike):
    """Value and standard error of a European call under a LOCAL-VOLATILITY surface σ(t, S) by Monte-Carlo: the log-Euler scheme
    X_{i+1} = X_i + (r − σ_i²/2) Δt_i + σ_i ΔW_i with σ_i = σ(t_i, S_i), S = exp(X); payoff max(S_T − K, 0) / exp(r T).
    The surface is tabulated: vols[j][k] = σ(times[j], spots[k]), piecewise constant in time (step i takes the last row whose time is not
    after t_i, the first row before that), linear in the spot with constant extrapolation.  σ_i is that row applied to S by
    RandomVariable.apply (tabulated.py): the state never leaves the device.  `maturity` must be a point of the time discretisation."""
    import numpy as np
    from .tabulated import TabulatedFunction
    times = np.asarray(times, dtype=np.float64).ravel()
    vols = np.asarray(vols, dtype=np.float64).reshape(times.size, -1)
    slices = {}
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw = brownian_motion.getBrownianIncrement(i, 0)
        row = max(int(np.searchsorted(times, t + 1e-12, side="right")) - 1, 0)
        if row not in slices: slices[row] = TabulatedFunction(spots, vols[row], "linear", "constant")
        sigma = x.exp().apply(slices[row])
        x = x.add(sigma.squared().mult(-0.5 * dt).add(risk_free_rate * dt)).addProduct(sigma, dw)
        i += 1
        t = td.getTime(i)
    value = x.exp().sub(strike).floor(0.0).div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value.getStandardError()


def geometric_asian_call_mc(brownian_motion, initial_value, risk_free_rate, volatility, maturity, strike):
    """Value of a call on the geometric average G = exp(mean of ln S(t_k), k = 1 … n) over the points of the time discretisation up to
    `maturity` (the initial time excluded) under Black–Scholes by Monte-Carlo: the log-Euler scheme of black_scholes_call_mc, which is
    exact for ln S; payoff max(G - K, 0) / exp(r T).  Written in RandomVariable methods only."""
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    total = None
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw = brownian_motion.getBrownianIncrement(i, 0)
        x = x.add((risk_free_rate - 0.5 * volatility * volatility) * dt).addProduct(dw, volatility)
        total = x if total is None else total.add(x)
        i += 1
        t = td.getTime(i)
    payoff = total.div(float(i)).exp().sub(strike).floor(0.0)
    value = payoff.div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value


def geometric_asian_call_analytic(initial_value, risk_free_rate, volatility, times, strike):
    """Closed form of geometric_asian_call_mc: `times` = the monitoring times t_1 … t_n (maturity t_n).  ln G is normal with mean
    ln S0 + (r - σ²/2) · mean(t_k) and variance σ² / n² · Σ_i Σ_j min(t_i, t_j)."""
    from math import erf, exp, log, sqrt
    ts = [float(t) for t in times]
    n = len(ts)
    mean = log(initial_value) + (risk_free_rate - 0.5 * volatility ** 2) * sum(ts) / n
    variance = volatility ** 2 / (n * n) * sum((2 * (n - k) - 1) * t for k, t in enumerate(sorted(ts)))
    cdf = lambda z: 0.5 * (1.0 + erf(z / sqrt(2.0)))
    d2 = (mean - log(strike)) / sqrt(variance)
    d1 = d2 + sqrt(variance)
    return exp(-risk_free_rate * ts[-1]) * (exp(mean + 0.5 * variance) * cdf(d1) - strike * cdf(d2))


def merton_call_mc(increments, initial_value, risk_free_rate, volatility, jump_intensity, jump_size_mean, jump_size_stddev, maturity, strike):
    """Value of a European call under Merton's jump-diffusion by Monte-Carlo, log-Euler scheme: per time step
    X += (r - σ²/2 - λ(e^{μ+δ²/2} - 1)) Δt + σ ΔW + μ ΔN + δ sqrt(ΔN) Z,  S = exp(X),
    with ΔW = increments(i, 0) (normal, sqrt(Δt)), Z = increments(i, 1) (standard normal), ΔN = increments(i, 2) (Poisson, mean λ Δt):
    given ΔN jumps their log sizes sum to a normal with mean μ ΔN and variance δ² ΔN, so one normal draw serves any jump count.
    Written in RandomVariable methods only.  `maturity` must be a point of the time discretisation."""
    td = increments.getTimeDiscretization()
    x = increments.getRandomVariableForConstant(math.log(initial_value))
    compensator = jump_intensity * (math.exp(jump_size_mean + 0.5 * jump_size_stddev * jump_size_stddev) - 1.0)
    drift = risk_free_rate - 0.5 * volatility * volatility - compensator
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw, z, dn = increments.getIncrement(i, 0), increments.getIncrement(i, 1), increments.getIncrement(i, 2)
        x = x.add(drift * dt).addProduct(dw, volatility).addProduct(dn, jump_size_mean).addProduct(dn.sqrt().mult(z), jump_size_stddev)
        i += 1
        t = td.getTime(i)
    payoff = x.exp().sub(strike).floor(0.0)
    value = payoff.div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value


def merton_call_by_jump_count_mc(increments, initial_value, risk_free_rate, volatility, jump_intensity, jump_size_mean, jump_size_stddev, maturity, strike,
                                 max_jumps=15):
    """Merton's series, term by term, by Monte-Carlo: merton_call_mc's simulation, the Poisson factor summed over the time steps to the
    number of jumps N_T per path (exact small integers), and the discounted payoff grouped by it on the device (group.py, DESIGN.md
    §4.29).  Returns a dict of lists over k = 0 … max_jumps — "share" (the fraction of paths with N_T = k: the Poisson probability),
    "mean" (E[discounted payoff | N_T = k]: e^{-rT}·Black(F_k, K, σ²T + kδ²), NaN for a count of 0), "standard_error" (of that mean),
    "count" — and "ungrouped", the number of paths with more than max_jumps jumps."""
    from .group import group_moments
    td = increments.getTimeDiscretization()
    x = increments.getRandomVariableForConstant(math.log(initial_value))
    compensator = jump_intensity * (math.exp(jump_size_mean + 0.5 * jump_size_stddev * jump_size_stddev) - 1.0)
    drift = risk_free_rate - 0.5 * volatility * volatility - compensator
    jumps = None
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw, z, dn = increments.getIncrement(i, 0), increments.getIncrement(i, 1), increments.getIncrement(i, 2)
        x = x.add(drift * dt).addProduct(dw, volatility).addProduct(dn, jump_size_mean).addProduct(dn.sqrt().mult(z), jump_size_stddev)
        jumps = dn if jumps is None else jumps.add(dn)
        i += 1
        t = td.getTime(i)
    value = x.exp().sub(strike).floor(0.0).div(math.exp(risk_free_rate * maturity))
    ((mean, variance),), counts, ungrouped = group_moments(jumps, [value], max_jumps + 1, what=("mean", "variance"), counts=True)
    count = [float(c) for c in counts.realizations.to_float32()]
    mean = [float(v) for v in mean.realizations.to_float32()]
    variance = [float(v) for v in variance.realizations.to_float32()]
    paths = sum(count) + ungrouped
    return {"share": [c / paths for c in count], "mean": mean, "count": count, "ungrouped": ungrouped,
            "standard_error": [math.sqrt(v / c) if c > 0 else math.nan for v, c in zip(variance, count)]}


def merton_call_analytic(initial_value, risk_free_rate, volatility, jump_intensity, jump_size_mean, jump_size_stddev, maturity, strike):
    """Merton (1976): the call is a Poisson mixture of Black–Scholes prices.  With m = e^{μ+δ²/2}, λ' = λ m: Σ_n e^{-λ'T} (λ'T)^n / n! ·
    BS(S, K, r_n, σ_n, T),  σ_n² = σ² + n δ² / T,  r_n = r - λ(m - 1) + n (μ + δ²/2) / T; summed until the weight is below 1e-16
    past the mode."""
    m = math.exp(jump_size_mean + 0.5 * jump_size_stddev * jump_size_stddev)
    lam = jump_intensity * m * maturity
    weight, total, n = math.exp(-lam), 0.0, 0
    while True:
        sigma_n = math.sqrt(volatility * volatility + n * jump_size_stddev * jump_size_stddev / maturity)
        r_n = risk_free_rate - jump_intensity * (m - 1.0) + n * (jump_size_mean + 0.5 * jump_size_stddev * jump_size_stddev) / maturity
        # BS with rate r_n discounts by e^{-r_n T}: the value under the mixture is that price as it stands (Merton's formula)
        total += weight * black_scholes_call_analytic(initial_value, r_n, sigma_n, maturity, strike)
        n += 1
        weight *= lam / n
        if n > lam and weight < 1e-16:
            return total


def heston_call_analytic(initial_value, risk_free_rate, v0, kappa, theta, xi, rho, maturity, strike, **node_arguments):
    """Heston (1993) by Lewis' single integral: transform.heston_call_analytic, the host definition of the device's transform pass at a
    number.  What heston_call_mc and heston_call_conditional_mc estimate, but for their Euler bias."""
    from .transform import heston_call_analytic as at_a_number
    return at_a_number(initial_value, risk_free_rate, v0, kappa, theta, xi, rho, maturity, strike, **node_arguments)


def variance_gamma_martingale_correction(sigma, theta, nu):
    """ω = ln(1 − θν − σ²ν/2)/ν:  E exp(X_t) = exp(−ω t) for the variance-gamma process X, so S = S₀ exp((r + ω) t + X_t) is a martingale
    after discounting."""
    taken = theta * nu + 0.5 * sigma * sigma * nu                       # small for a small ν: log1p keeps its digits
    if not taken < 1.0: raise ValueError("1 - theta nu - sigma^2 nu / 2 must be positive")
    return math.log1p(-taken) / nu


def variance_gamma_call_mc(process, initial_value, risk_free_rate, maturity, strike):
    """Value of a European call under the variance-gamma model by Monte-Carlo: per time step X += (r + ω) Δt + ΔV, S = exp(X), ΔV =
    process.getIncrement(i, 0) = θ ΔΓ + σ sqrt(ΔΓ) Z (increments.VarianceGammaProcess), ω the martingale correction.  Written in
    RandomVariable methods only.  `maturity` must be a point of the time discretisation."""
    td = process.getTimeDiscretization()
    x = process.getRandomVariableForConstant(math.log(initial_value))
    drift = risk_free_rate + variance_gamma_martingale_correction(process.sigma, process.theta, process.nu)
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        x = x.add(drift * td.getTimeStep(i)).add(process.getIncrement(i, 0))
        i += 1
        t = td.getTime(i)
    payoff = x.exp().sub(strike).floor(0.0)
    value = payoff.div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value


def variance_gamma_call_analytic(initial_value, risk_free_rate, sigma, theta, nu, maturity, strike, nodes=400):
    """Given the gamma time g = Γ_T ~ Gamma(T/ν, ν), ln S_T is normal with mean ln S₀ + (r + ω) T + θ g and variance σ² g: the call is a
    Black–Scholes price with forward F(g) = S₀ exp((r + ω) T + θ g + σ² g / 2) and total variance σ² g, and the value is its integral
    against the gamma density.  With g = ν y the integral is ∫ y^(α−1) e^(−y) h(y) dy / Γ(α), α = T/ν: Gauss–Laguerre quadrature with
    weight y^(α−1) e^(−y) — nodes and weights from the Jacobi matrix of the generalised Laguerre polynomials (Golub–Welsch), in numpy —
    which takes the density's singularity at 0 (α < 1) into the weight."""
    import numpy as np
    alpha = maturity / nu
    omega = variance_gamma_martingale_correction(sigma, theta, nu)
    k = np.arange(nodes, dtype=np.float64)
    diagonal = 2.0 * k + alpha                                           # recurrence of L_n^(α−1): a_k = 2k + α, b_k² = k (k + α − 1)
    off = np.sqrt(k[1:] * (k[1:] + alpha - 1.0))
    y, vectors = np.linalg.eigh(np.diag(diagonal) + np.diag(off, 1) + np.diag(off, -1))
    weights = vectors[0] ** 2                                             # normalised: they sum to 1 = ∫ density
    total = 0.0
    discount = math.exp(-risk_free_rate * maturity)
    sqrt2 = math.sqrt(2.0)
    for yi, wi in zip(y, weights):
        g = nu * yi
        if not g > 0.0 or wi < 1e-300: continue
        forward = initial_value * math.exp((risk_free_rate + omega) * maturity + theta * g + 0.5 * sigma * sigma * g)
        s = sigma * math.sqrt(g)
        d1 = (math.log(forward / strike) + 0.5 * s * s) / s
        d2 = d1 - s
        total += wi * discount * (forward * 0.5 * (1.0 + math.erf(d1 / sqrt2)) - strike * 0.5 * (1.0 + math.erf(d2 / sqrt2)))
    return total


def heston_call_mc(brownian_motion, initial_value, risk_free_rate, v0, kappa, theta, xi, rho, maturity, strike):
    """Euler full-truncation Heston:  v⁺ = max(v, 0);
        X_{i+1} = X_i + (r - v⁺/2) Δt + sqrt(v⁺) ΔW¹
        v_{i+1} = v_i + κ(θ - v⁺) Δt + ξ sqrt(v⁺) (ρ ΔW¹ + sqrt(1-ρ²) ΔW²)
    Uses factors 0 and 1 of the Brownian motion.  ξ = 0, v0 = θ reduces to Black–Scholes with σ² = θ."""
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    v = brownian_motion.getRandomVariableForConstant(v0)
    rho_c = math.sqrt(1.0 - rho * rho)
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw1 = brownian_motion.getBrownianIncrement(i, 0)
        dw2 = brownian_motion.getBrownianIncrement(i, 1)
        vp = v.floor(0.0)
        sq = vp.sqrt()
        x = x.add(risk_free_rate * dt).addProduct(vp, -0.5 * dt).addProduct(sq, dw1)
        if xi != 0.0:
            dz = dw1.mult(rho).addProduct(dw2, rho_c)
            v = v.addProduct(vp.bus(theta), kappa * dt).addProduct(sq.mult(xi), dz)
        else:
            v = v.addProduct(vp.bus(theta), kappa * dt)
        i += 1
        t = td.getTime(i)
    payoff = x.exp().sub(strike).floor(0.0)
    value = payoff.div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value


def heston_call_conditional_mc(brownian_motion, initial_value, risk_free_rate, v0, kappa, theta, xi, rho, maturity, strike):
    """CONDITIONAL Monte-Carlo ("mixing") for heston_call_mc's scheme: only the variance is simulated,
        v_{i+1} = v_i + κ(θ − v⁺) Δt + ξ sqrt(v⁺) ΔZ,   v⁺ = max(v, 0),   ΔZ = factor 0 of the Brownian motion,
    with I = Σ v⁺ Δt and J = Σ sqrt(v⁺) ΔZ accumulated along the path.  Given the path of Z, the Euler log-price
    X_T = ln S₀ + rT − I/2 + ρ J + sqrt(1 − ρ²) Σ sqrt(v⁺) ΔW^⊥ is normal: the payoff's conditional expectation is the Black–Scholes value
        black_scholes_option_value(S₀ e^{rT} exp(ρ J − ρ² I / 2), sqrt((1 − ρ²) I / T), T, K, e^{−rT})
    per path (analytic.py, DESIGN.md §4.21: one launch on the three vectors, nothing leaves the device).  This is the exact conditional law
    of the Euler scheme, so the average has the expectation of heston_call_mc's, with less variance.  Returns (average, vector)."""
    from .analytic import black_scholes_option_value
    td = brownian_motion.getTimeDiscretization()
    v = brownian_motion.getRandomVariableForConstant(v0)
    integral = brownian_motion.getRandomVariableForConstant(0.0)
    stochastic = brownian_motion.getRandomVariableForConstant(0.0)
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dz = brownian_motion.getBrownianIncrement(i, 0)
        vp = v.floor(0.0)
        sq = vp.sqrt()
        integral = integral.addProduct(vp, dt)
        stochastic = stochastic.addProduct(sq, dz)
        if xi != 0.0:
            v = v.addProduct(vp.bus(theta), kappa * dt).addProduct(sq.mult(xi), dz)
        else:
            v = v.addProduct(vp.bus(theta), kappa * dt)
        i += 1
        t = td.getTime(i)
    forward = stochastic.mult(rho).addProduct(integral, -0.5 * rho * rho).exp().mult(initial_value * math.exp(risk_free_rate * maturity))
    volatility = integral.mult((1.0 - rho * rho) / maturity).sqrt()
    value = black_scholes_option_value(forward, volatility, maturity, strike, math.exp(-risk_free_rate * maturity))
    return value.getAverage(), value


def forward_implied_volatility_mc(brownian_motion_outer, brownian_motion_inner, inner_paths, initial_value, risk_free_rate, v0, kappa, theta, xi, rho, time, maturity,
                                  moneyness=(1.0,), quantiles=(0.05, 0.5, 0.95)):
    """The distribution, at `time`, of the Black–Scholes volatility implied by the price of a call expiring at `maturity` under
    heston_call_mc's scheme — the FORWARD SMILE — by nested simulation.  Returns one dict per moneyness m: {"moneyness", "mean",
    "standard_error", "quantiles" (getQuantile at each of `quantiles`, in its convention: the value that this fraction of the paths exceeds),
    "not_invertible"}.
    OUTER: the paths of brownian_motion_outer carry (S, v) from the first point of its time discretisation to `time` (a point of it).
    INNER: inner_paths paths per outer state (nested.repeat_each) carry both on over the steps of brownian_motion_inner until
    maturity − time has passed (a point of its discretisation, counted from its first).  Per outer path the inner payoffs at the strike
    m·S_t·exp(r(T − t)) — moneyness m of the forward at t — are reduced by nested.block_means to the undiscounted forward price of the call,
    and analytic.implied_volatility inverts it with that per-path strike and the maturity T − t.
    "not_invertible" is the share of outer paths whose implied volatility is NaN or 0 (an inner mean at or outside the bounds); mean,
    standard error and quantiles are those of the other paths.  Nothing leaves the device but these numbers.  FMHIP_DEVICE_NESTED=0 and
    FMHIP_DEVICE_ANALYTIC=0 give the same numbers to the last bit: the host definitions are the device's."""
    from .analytic import implied_volatility
    from .nested import block_means, repeat_each
    inner_paths = int(inner_paths)
    if inner_paths < 1: raise ValueError("at least one inner path per outer path")
    if brownian_motion_inner.getNumberOfPaths() != brownian_motion_outer.getNumberOfPaths() * inner_paths:
        raise ValueError("the inner Brownian motion has not inner_paths paths per outer path")
    if not maturity > time: raise ValueError("the option expires after the time at which its volatility is implied")
    rho_c = math.sqrt(1.0 - rho * rho)

    def advance(bm, x, v, span):                                                # heston_call_mc's step
        td = bm.getTimeDiscretization()
        start, i = td.getTime(0), 0
        while td.getTime(i) - start < span - 1e-12:
            dt = td.getTimeStep(i)
            dw1 = bm.getBrownianIncrement(i, 0)
            vp = v.floor(0.0)
            sq = vp.sqrt()
            x = x.add(risk_free_rate * dt).addProduct(vp, -0.5 * dt).addProduct(sq, dw1)
            if xi != 0.0:
                dz = dw1.mult(rho).addProduct(bm.getBrownianIncrement(i, 1), rho_c)
                v = v.addProduct(vp.bus(theta), kappa * dt).addProduct(sq.mult(xi), dz)
            else:
                v = v.addProduct(vp.bus(theta), kappa * dt)
            i += 1
        if abs(td.getTime(i) - start - span) > 1e-12: raise ValueError("the horizon is not a point of the time discretisation")
        return x, v

    t0 = brownian_motion_outer.getTimeDiscretization().getTime(0)
    x, v = advance(brownian_motion_outer, brownian_motion_outer.getRandomVariableForConstant(math.log(initial_value)),
                   brownian_motion_outer.getRandomVariableForConstant(v0), time - t0)
    x_inner, _ = advance(brownian_motion_inner, repeat_each(x, inner_paths), repeat_each(v, inner_paths), maturity - time)
    forward = x.exp().mult(math.exp(risk_free_rate * (maturity - time)))
    terminal = x_inner.exp()
    one, zero = forward.mult(0.0).add(1.0), forward.mult(0.0)
    n_outer = brownian_motion_outer.getNumberOfPaths()
    results = []
    for m in moneyness:
        strike = forward.mult(float(m))
        price = block_means(terminal.sub(repeat_each(strike, inner_paths)).floor(0.0), inner_paths)
        sigma, = implied_volatility("black_scholes", price, forward, maturity - time, strike)
        valid = sigma.choose(one, zero).mult(sigma.mult(-1.0).choose(zero, one))       # 1 where sigma > 0, 0 where it is 0 or a NaN
        clean = valid.sub(0.5).choose(sigma, zero)
        share = valid.getAverage()
        if share > 0.0:
            mean = clean.getAverage() / share
            variance = max(clean.squared().getAverage() / share - mean * mean, 0.0)
            error = math.sqrt(variance / (n_outer * share))
            levels = [clean.getQuantile(q * share) for q in quantiles]     # getQuantile(q): the value that the fraction q of the sample exceeds; the invalid paths are the zeros at the bottom
        else:
            mean, error, levels = math.nan, math.nan, [math.nan for _ in quantiles]
        results.append({"moneyness": float(m), "mean": mean, "standard_error": error, "quantiles": levels, "not_invertible": 1.0 - share})
    return results


def forward_implied_volatility_transform_mc(brownian_motion_outer, initial_value, risk_free_rate, v0, kappa, theta, xi, rho, time, maturity,
                                            moneyness=(1.0,), quantiles=(0.05, 0.5, 0.95), **node_arguments):
    """forward_implied_volatility_mc without the inner simulation: the OUTER paths are its own (heston_call_mc's scheme carries (S, v) from the
    first point of brownian_motion_outer's time discretisation to `time`, a point of it), and the price of the call expiring at `maturity`
    at the strike m·S_t·exp(r(T − t)) is the model's — transform.heston_option_value on the forward S_t·exp(r(T − t)) and the variance
    v_t⁺ = max(v_t, 0) of every path for the maturity T − t (one node table, one launch per moneyness) — which analytic.implied_volatility
    inverts with that per-path strike.  The same dicts: {"moneyness", "mean", "standard_error", "quantiles", "not_invertible"}.  No inner paths,
    no inner noise, no inner Euler bias; what is left in "not_invertible" is a time value below the fp32 rounding of the price.  ξ > 0 (the
    transform of Heston's model has no ξ = 0 form).  node_arguments go to transform.heston_transform_nodes."""
    from .analytic import implied_volatility
    from .transform import heston_transform_nodes, transform_option_value
    if not maturity > time: raise ValueError("the option expires after the time at which its volatility is implied")
    rho_c = math.sqrt(1.0 - rho * rho)
    td = brownian_motion_outer.getTimeDiscretization()
    x = brownian_motion_outer.getRandomVariableForConstant(math.log(initial_value))
    v = brownian_motion_outer.getRandomVariableForConstant(v0)
    start, i = td.getTime(0), 0
    while td.getTime(i) - start < time - start - 1e-12:                        # heston_call_mc's step
        dt = td.getTimeStep(i)
        dw1 = brownian_motion_outer.getBrownianIncrement(i, 0)
        vp = v.floor(0.0)
        sq = vp.sqrt()
        x = x.add(risk_free_rate * dt).addProduct(vp, -0.5 * dt).addProduct(sq, dw1)
        dz = dw1.mult(rho).addProduct(brownian_motion_outer.getBrownianIncrement(i, 1), rho_c)
        v = v.addProduct(vp.bus(theta), kappa * dt).addProduct(sq.mult(xi), dz)
        i += 1
    if abs(td.getTime(i) - time) > 1e-12: raise ValueError("the horizon is not a point of the time discretisation")
    nodes = heston_transform_nodes(kappa, theta, xi, rho, maturity - time, **node_arguments)
    forward = x.exp().mult(math.exp(risk_free_rate * (maturity - time)))
    variance = v.floor(0.0)
    one, zero = forward.mult(0.0).add(1.0), forward.mult(0.0)
    n_outer = brownian_motion_outer.getNumberOfPaths()
    results = []
    for m in moneyness:
        strike = forward.mult(float(m))
        price, = transform_option_value(nodes, forward, (variance,), strike)
        sigma, = implied_volatility("black_scholes", price, forward, maturity - time, strike)
        valid = sigma.choose(one, zero).mult(sigma.mult(-1.0).choose(zero, one))       # 1 where sigma > 0, 0 where it is 0 or a NaN
        clean = valid.sub(0.5).choose(sigma, zero)
        share = valid.getAverage()
        if share > 0.0:
            mean = clean.getAverage() / share
            variance_of = max(clean.squared().getAverage() / share - mean * mean, 0.0)
            error = math.sqrt(variance_of / (n_outer * share))
            levels = [clean.getQuantile(q * share) for q in quantiles]
        else:
            mean, error, levels = math.nan, math.nan, [math.nan for _ in quantiles]
        results.append({"moneyness": float(m), "mean": mean, "standard_error": error, "quantiles": levels, "not_invertible": 1.0 - share})
    return results


def stochastic_local_volatility_call_mc(brownian_motion, initial_value, risk_free_rate, times, spots, dupire_vols, v0, kappa, theta, xi, rho, maturity, strike,
                                        n_points=64, order=0):
    """Value and standard error of a European call under a LOCAL-STOCHASTIC-VOLATILITY model calibrated on the fly by the particle method
    (Guyon, Henry-Labordère): heston_call_mc's variance scheme (Euler, full truncation), local_volatility_call_mc's surface lookup, and the
    leverage function L(t_i, S)² = σ_Dupire(t_i, S)² / max(E[v⁺_i | ln S_i], 1e-8), re-estimated at EVERY time step by kernel regression
    on X = ln S (kernel_regression.py, DESIGN.md §4.19: Epanechnikov, n_points uniform points between the 0.1 % and 99.9 % quantiles of X,
    bandwidth max(3 · Silverman, 1.5 · spacing), local constant or local linear fit, linear interpolation between the points):
        a_i² = L_i² v⁺_i,   X_{i+1} = X_i + (r − a_i²/2) Δt + a_i ΔW¹,   v_{i+1} = v_i + κ(θ − v⁺_i) Δt + ξ sqrt(v⁺_i) (ρ ΔW¹ + sqrt(1−ρ²) ΔW²).
    Step 0, where the state is a constant, uses σ²/v0.  A deterministic variance (ξ = 0) is its own conditional expectation: the model is
    then the local-volatility model of the surface.  Written in RandomVariable methods, kernel_moments and apply only: per step nothing
    leaves the device but two quantiles, a variance and the n_points sums.  Uses factors 0 and 1 of the Brownian motion; `maturity` must be
    a point of the time discretisation."""
    import numpy as np
    from .kernel_regression import MonteCarloConditionalExpectationKernelRegression
    from .tabulated import TabulatedFunction
    times = np.asarray(times, dtype=np.float64).ravel()
    vols = np.asarray(dupire_vols, dtype=np.float64).reshape(times.size, -1)
    slices = {}
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    v = brownian_motion.getRandomVariableForConstant(v0)
    rho_c = math.sqrt(1.0 - rho * rho)
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        dt = td.getTimeStep(i)
        dw1 = brownian_motion.getBrownianIncrement(i, 0)
        row = max(int(np.searchsorted(times, t + 1e-12, side="right")) - 1, 0)
        if row not in slices: slices[row] = TabulatedFunction(spots, vols[row], "linear", "constant")
        dupire_variance = x.exp().apply(slices[row]).squared()
        vp = v.floor(0.0)
        if vp.isDeterministic(): conditional = vp                  # E[v⁺ | X] of a constant (step 0: v0)
        elif x.isDeterministic(): conditional = vp.average()
        else: conditional = MonteCarloConditionalExpectationKernelRegression(x, n_points, None, "epanechnikov", order).getConditionalExpectation(vp)
        variance = dupire_variance.mult(vp).div(conditional.floor(1e-8))      # a² = σ² v⁺ / max(E[v⁺ | X], 1e-8)
        x = x.add(risk_free_rate * dt).addProduct(variance, -0.5 * dt).addProduct(variance.sqrt(), dw1)
        if xi != 0.0:
            dw2 = brownian_motion.getBrownianIncrement(i, 1)
            dz = dw1.mult(rho).addProduct(dw2, rho_c)
            v = v.addProduct(vp.bus(theta), kappa * dt).addProduct(vp.sqrt().mult(xi), dz)
        else:
            v = v.addProduct(vp.bus(theta), kappa * dt)
        i += 1
        t = td.getTime(i)
    value = x.exp().sub(strike).floor(0.0).div(math.exp(risk_free_rate * maturity))
    return value.getAverage(), value.getStandardError()


def bermudan_option_mc(brownian_motion, initial_value, risk_free_rate, volatility, exercise_dates, strike, call=False, basis_order=3, bins=0, in_the_money_only=False):
    """Value of a Bermudan option under Black–Scholes by Longstaff–Schwartz backward induction.  States from the log-Euler scheme of
    black_scholes_call_mc, kept at the exercise dates (points of the time discretisation).  The value starts as the last date's discounted
    payoff; at each earlier date the current value is regressed on 1, S, …, S^basis_order over ALL paths (the constant is a deterministic
    random variable: a host scalar to the estimator), and paths on which exercise − continuation estimate >= 0 take the discounted exercise
    value.  Returns (value.getAverage(), value).  With one exercise date this is the European option on the same paths.
    bins > 0: the regression is LOCALIZED — per quantile bin of S (bins of equal count, at most 64) on 1, S, …, S^basis_order with
    basis_order <= 2 (MonteCarloConditionalExpectationLocalizedRegression); bins = 0: the global fit.
    in_the_money_only=True: Longstaff & Schwartz's regression over the paths on which exercise is worth something.  At
    each date the mask is strike − S (put) or S − strike (call); the state and the current value are compressed by it
    (selection.compress), the estimator fits and evaluates on the short vectors, and the estimate is expanded back with fill = +inf, so
    that exercise − continuation is −inf on the other paths and choose keeps the value there.  A date on which no path is selected
    leaves the value as it is.  A cubic then suffices where the all-paths fit needs degree 5."""
    from .regression import MonteCarloConditionalExpectationLocalizedRegression, MonteCarloConditionalExpectationRegression
    from .selection import compress, expand
    if bins and basis_order + 1 > 3: raise ValueError("a localized regression takes at most 3 basis functions per bin: basis_order <= 2")
    dates = sorted(float(d) for d in exercise_dates)
    if not dates: raise ValueError("no exercise date")
    td = brownian_motion.getTimeDiscretization()
    x = brownian_motion.getRandomVariableForConstant(math.log(initial_value))
    states, t, i = [], td.getTime(0), 0
    if abs(t - dates[0]) <= 1e-12: states.append(x.exp())
    while len(states) < len(dates):
        dt = td.getTimeStep(i)
        dw = brownian_motion.getBrownianIncrement(i, 0)
        x = x.add((risk_free_rate - 0.5 * volatility * volatility) * dt).addProduct(dw, volatility)
        i += 1
        t = td.getTime(i)
        if t > dates[len(states)] + 1e-12: raise ValueError("an exercise date is not a point of the time discretisation")
        if abs(t - dates[len(states)]) <= 1e-12: states.append(x.exp())

    def exercise_value(s, date):
        payoff = s.sub(strike).floor(0.0) if call else s.bus(strike).floor(0.0)
        return payoff.div(math.exp(risk_free_rate * date))

    value = exercise_value(states[-1], dates[-1])
    one = brownian_motion.getRandomVariableForConstant(1.0)
    for k in range(len(dates) - 2, -1, -1):
        s = states[k]
        if in_the_money_only:
            mask = s.sub(strike) if call else s.bus(strike)
            (short_s, short_value), count = compress(mask, [s, value])
            if count == 0: continue
            basis = [one, short_s]
            for _ in range(2, basis_order + 1): basis.append(basis[-1].mult(short_s))
            basis = basis[:basis_order + 1]
            if bins: estimate = MonteCarloConditionalExpectationLocalizedRegression(short_s, bins, basis).getConditionalExpectation(short_value)
            else: estimate = MonteCarloConditionalExpectationRegression(basis).getConditionalExpectation(short_value)
            (continuation,) = expand(mask, [estimate], fill=math.inf)
            exercise = exercise_value(s, dates[k])
            value = exercise.sub(continuation).choose(exercise, value)
            continue
        basis = [one, s]
        for _ in range(2, basis_order + 1): basis.append(basis[-1].mult(s))
        basis = basis[:basis_order + 1]
        if bins: continuation = MonteCarloConditionalExpectationLocalizedRegression(s, bins, basis).getConditionalExpectation(value)
        else: continuation = MonteCarloConditionalExpectationRegression(basis).getConditionalExpectation(value)
        exercise = exercise_value(s, dates[k])
        value = exercise.sub(continuation).choose(exercise, value)
    return value.getAverage(), value


def bermudan_option_bounds_mc(brownian_motion_fit, brownian_motion_outer, inner_paths, inner_seed, initial_value, risk_free_rate, volatility,
                              exercise_dates, strike, call=False, basis_order=3):
    """Primal–dual bounds of a Bermudan option under Black–Scholes (Andersen & Broadie 2004); model, scheme and payoff of bermudan_option_mc,
    whose in-sample value is neither bound.  Returns dict(lower, lower_se, upper, upper_se), all discounted to time 0.
    POLICY: the coefficients β_j of the continuation value on 1, S, …, S^basis_order come from the FIT sample by getLinearRegressionParameters
    at each date, backwards, exactly as bermudan_option_mc regresses; a path stops at the first date j with h_j − Σβ_{j,i}S^i >= 0, and at the
    last date always.
    LOWER: the mean, over the OUTER sample (independent of the fit sample), of the discounted payoff at the policy's stopping date.
    UPPER: for j = −1 (the root) and every date j = 0 … J−2, inner_paths inner paths are started from each outer path's state at j
    (nested.repeat_each; a Brownian motion of m·inner_paths paths seeded inner_seed + j + 1) and follow the policy from date j+1 on; the
    block mean of their discounted payoffs is C_j, an unbiased estimate of E_j[V_{j+1}] (nested.block_means).  V_j = h_j where the policy
    stops at j (and at the last date), else C_j; M_{−1} = 0, M_j = M_{j−1} + V_j − C_{j−1}; upper = mean(max_j(h_j − M_j)).  The inner noise
    biases the upper bound upwards, by less with more inner paths.  The standard errors are taken over the outer paths.
    With FMHIP_DEVICE_NESTED=0 the four numbers are the same to the last bit: the host definition of the block means is the device's."""
    import numpy as np
    from .brownian_motion import BrownianMotionHip, TimeDiscretization
    from .nested import block_means, repeat_each
    from .regression import MonteCarloConditionalExpectationRegression
    dates = sorted(float(d) for d in exercise_dates)
    if not dates: raise ValueError("no exercise date")
    inner_paths = int(inner_paths)
    if inner_paths < 1: raise ValueError("at least one inner path per outer path")
    drift = risk_free_rate - 0.5 * volatility * volatility

    def states_at(bm, x, wanted):
        """[(log state, state) at each date of `wanted`] by the log-Euler scheme from x at the first time of bm's discretisation."""
        td = bm.getTimeDiscretization()
        out, t, i = [], td.getTime(0), 0
        if wanted and abs(t - wanted[0]) <= 1e-12: out.append((x, x.exp()))
        while len(out) < len(wanted):
            x = x.add(drift * td.getTimeStep(i)).addProduct(bm.getBrownianIncrement(i, 0), volatility)
            i += 1
            t = td.getTime(i)
            if t > wanted[len(out)] + 1e-12: raise ValueError("an exercise date is not a point of the time discretisation")
            if abs(t - wanted[len(out)]) <= 1e-12: out.append((x, x.exp()))
        return out

    def exercise_value(s, date):
        payoff = s.sub(strike).floor(0.0) if call else s.bus(strike).floor(0.0)
        return payoff.div(math.exp(risk_free_rate * date))

    def continuation(s, beta, one):
        ce = one.mult(float(beta[0]))
        power = s
        for i in range(1, len(beta)):
            ce = ce.addProduct(power, float(beta[i]))
            if i + 1 < len(beta): power = power.mult(s)
        return ce

    def policy_value(states, first, one):
        """The discounted payoff at the policy's stopping date, for paths that are alive at date `first`; states[k - first] = S at date k."""
        value = exercise_value(states[-1], dates[-1])
        for k in range(len(dates) - 2, first - 1, -1):
            exercise = exercise_value(states[k - first], dates[k])
            value = exercise.sub(continuation(states[k - first], betas[k], one)).choose(exercise, value)
        return value

    # the policy, from the fit sample
    one = brownian_motion_fit.getRandomVariableForConstant(1.0)
    fit = [s for _, s in states_at(brownian_motion_fit, brownian_motion_fit.getRandomVariableForConstant(math.log(initial_value)), dates)]
    betas = [None] * len(dates)
    value = exercise_value(fit[-1], dates[-1])
    for k in range(len(dates) - 2, -1, -1):
        s = fit[k]
        basis = [one, s]
        for _ in range(2, basis_order + 1): basis.append(basis[-1].mult(s))
        basis = basis[:basis_order + 1]
        betas[k] = MonteCarloConditionalExpectationRegression(basis).getLinearRegressionParameters(value)
        exercise = exercise_value(s, dates[k])
        value = exercise.sub(continuation(s, betas[k], one)).choose(exercise, value)

    # the lower bound: the policy on the outer sample
    one = brownian_motion_outer.getRandomVariableForConstant(1.0)
    x0 = brownian_motion_outer.getRandomVariableForConstant(math.log(initial_value))
    outer = states_at(brownian_motion_outer, x0, dates)
    lower = policy_value([s for _, s in outer], 0, one)

    # the upper bound: the martingale from inner simulations at the root and at every date but the last
    m = brownian_motion_outer.getNumberOfPaths()
    times = brownian_motion_outer.getTimeDiscretization().getAsDoubleArray()
    previous_c, martingale, worst = None, None, None
    for j in range(-1, len(dates)):
        if j < len(dates) - 1:
            start_time = times[0] if j < 0 else dates[j]
            first_index = int(np.argmin(np.abs(times - start_time)))
            inner_bm = BrownianMotionHip(TimeDiscretization(times[first_index:]), 1, m * inner_paths, inner_seed + j + 1)
            start = x0 if j < 0 else repeat_each(outer[j][0], inner_paths)
            inner = states_at(inner_bm, start, dates[j + 1:])
            c = block_means(policy_value([s for _, s in inner], j + 1, one), inner_paths)
        else: c = None
        if j >= 0:
            h = exercise_value(outer[j][1], dates[j])
            v = h if c is None else h.sub(continuation(outer[j][1], betas[j], one)).choose(h, c)
            increment = v.sub(previous_c)
            martingale = increment if martingale is None else martingale.add(increment)
            gap = h.sub(martingale)
            worst = gap if worst is None else worst.floor(gap)
        previous_c = c
    return dict(lower=lower.getAverage(), lower_se=lower.getStandardError(), upper=worst.getAverage(), upper_se=worst.getStandardError())


def nested_initial_margin_mc(brownian_motion_outer, brownian_motion_inner, initial_value, risk_free_rate, volatility, time, margin_period, maturity, strike,
                             inner_paths, quantile=0.99):
    """Expected dynamic initial margin, at `time`, of a forward contract on a Black–Scholes asset by nested simulation: returns (E[IM], its
    standard error over the outer paths).
    OUTER: the m paths of brownian_motion_outer carry the log-Euler state from the first point of its time discretisation to `time` (a point
    of it).  INNER: inner_paths paths per outer state (nested.repeat_each) follow the same scheme over the steps of brownian_motion_inner —
    m·inner_paths paths — until `margin_period` has passed (a point of its discretisation, counted from its first).
    The contract's value at u is V(u) = S_u − K·exp(−r(T − u)); the inner P&L is V(time + margin_period) − V(time), per inner path, and
    IM = −getQuantile(quantile) of the inner P&L of each outer path (nested.block_quantiles: rank quantile_index(inner_paths, quantile) of
    the ascending block — the loss that the fraction `quantile` of the inner P&Ls does not exceed).  Nothing leaves the device but the two
    numbers.  With FMHIP_DEVICE_NESTED=0 they are the same to the last bit: the host definition of the block quantile is the device's."""
    from .nested import block_quantiles, repeat_each
    inner_paths = int(inner_paths)
    if inner_paths < 1: raise ValueError("at least one inner path per outer path")
    if brownian_motion_inner.getNumberOfPaths() != brownian_motion_outer.getNumberOfPaths() * inner_paths:
        raise ValueError("the inner Brownian motion has not inner_paths paths per outer path")
    drift = risk_free_rate - 0.5 * volatility * volatility

    def advance(bm, x, span):
        td = bm.getTimeDiscretization()
        start, i = td.getTime(0), 0
        while td.getTime(i) - start < span - 1e-12:
            x = x.add(drift * td.getTimeStep(i)).addProduct(bm.getBrownianIncrement(i, 0), volatility)
            i += 1
        if abs(td.getTime(i) - start - span) > 1e-12: raise ValueError("the horizon is not a point of the time discretisation")
        return x

    t0 = brownian_motion_outer.getTimeDiscretization().getTime(0)
    x = advance(brownian_motion_outer, brownian_motion_outer.getRandomVariableForConstant(math.log(initial_value)), time - t0)
    inner = advance(brownian_motion_inner, repeat_each(x, inner_paths), margin_period)
    value_change = strike * (math.exp(-risk_free_rate * (maturity - time - margin_period)) - math.exp(-risk_free_rate * (maturity - time)))
    pnl = inner.exp().sub(repeat_each(x.exp(), inner_paths)).sub(value_change)
    margin = block_quantiles(pnl, inner_paths, [quantile])[0].mult(-1.0)
    return margin.getAverage(), margin.getStandardError()


def monomial_exponents(n_assets, order):
    """All exponent tuples of total degree <= order in n_assets variables — C(n_assets + order, order) of them —, by degree, then
    lexicographically descending: (0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), …"""
    out = []
    def rest(prefix, left, slots):
        if slots == 1: out.append(tuple(prefix + [left])); return
        for e in range(left, -1, -1): rest(prefix + [e], left - e, slots - 1)
    for degree in range(order + 1): rest([], degree, n_assets)
    return out


def bermudan_max_call_mc(brownian_motion, initial_values, risk_free_rate, dividend_yield, volatility, exercise_dates, strike, basis_order=2, one_pass_basis=False,
                         ordered_states=False):
    """Value of a Bermudan call on max_i S_i under Black–Scholes by Longstaff–Schwartz backward induction: independent assets, asset i driven
    by factor i of `brownian_motion` (log-Euler, exact for ln S), drift r − δ − σ²/2, all with one dividend yield and one volatility.  States
    are kept at the exercise dates (points of the time discretisation).  The value starts as the last date's discounted payoff; at each
    earlier date it is regressed over ALL paths on all monomials of total degree <= basis_order in the assets, scaled by the strike —
    C(A + basis_order, basis_order) basis functions, the constant among them as a deterministic random variable — and paths on which
    exercise − continuation estimate >= 0 take the discounted exercise value.  One regression, that is one pass over the data on the device, per
    exercise date but the last.  Returns (value, standard error).  With one exercise date this is the European max-call on the same paths.
    one_pass_basis=True: the monomials are not built at all — MonteCarloConditionalExpectationPolynomialRegression forms them in registers
    from the scaled states.  The value is then the default's to the last bit wherever the default takes the wide pass
    (more than 12 basis functions); with 12 or fewer the default's narrow pass adds in another order and the two agree to rounding only.
    ordered_states=True: the scaled states of each exercise date are replaced by their order statistics across the assets, largest first
    (cross_section.sort_across, one launch per date: DESIGN.md §4.24), before the monomials are formed — the basis of ordered prices of
    Longstaff–Schwartz, Broadie–Glasserman and Andersen–Broadie, in which the exercise region of a max option is far closer to polynomial —
    on both routes, and the exercise value takes cross_section.max_across.  The default leaves the values as they were, bit for bit."""
    from .regression import MonteCarloConditionalExpectationPolynomialRegression, MonteCarloConditionalExpectationRegression
    from .cross_section import max_across, sort_across
    dates = sorted(float(d) for d in exercise_dates)
    if not dates: raise ValueError("no exercise date")
    assets = len(initial_values)
    if assets < 1 or assets > brownian_motion.getNumberOfFactors(): raise ValueError("one factor of the Brownian motion per asset")
    td = brownian_motion.getTimeDiscretization()
    xs = [brownian_motion.getRandomVariableForConstant(math.log(float(s0))) for s0 in initial_values]
    drift = risk_free_rate - dividend_yield - 0.5 * volatility * volatility
    states, t, i = [], td.getTime(0), 0
    if abs(t - dates[0]) <= 1e-12: states.append([x.exp() for x in xs])
    while len(states) < len(dates):
        dt = td.getTimeStep(i)
        xs = [x.add(drift * dt).addProduct(brownian_motion.getBrownianIncrement(i, a), volatility) for a, x in enumerate(xs)]
        i += 1
        t = td.getTime(i)
        if t > dates[len(states)] + 1e-12: raise ValueError("an exercise date is not a point of the time discretisation")
        if abs(t - dates[len(states)]) <= 1e-12: states.append([x.exp() for x in xs])

    def exercise_value(s, date):
        if ordered_states: best = max_across(s)
        else:
            best = s[0]
            for other in s[1:]: best = best.floor(other)         # max(best, other)
        return best.sub(strike).floor(0.0).div(math.exp(risk_free_rate * date))

    value = exercise_value(states[-1], dates[-1])
    one = brownian_motion.getRandomVariableForConstant(1.0)
    exponents = monomial_exponents(assets, basis_order)
    for k in range(len(dates) - 2, -1, -1):
        scaled = [s.div(strike) for s in states[k]]
        if ordered_states: scaled = sort_across(scaled, descending=True)
        if one_pass_basis:
            continuation = MonteCarloConditionalExpectationPolynomialRegression(scaled, exponents=exponents, one=one).getConditionalExpectation(value)
            exercise = exercise_value(states[k], dates[k])
            value = exercise.sub(continuation).choose(exercise, value)
            continue
        powers = [[one, u] for u in scaled]
        for p in powers:
            for _ in range(2, basis_order + 1): p.append(p[-1].mult(p[1]))
        basis = []
        for e in exponents:
            f = None
            for a, ea in enumerate(e):
                if ea: f = powers[a][ea] if f is None else f.mult(powers[a][ea])
            basis.append(one if f is None else f)
        continuation = MonteCarloConditionalExpectationRegression(basis).getConditionalExpectation(value)
        exercise = exercise_value(states[k], dates[k])
        value = exercise.sub(continuation).choose(exercise, value)
    return value.getAverage(), value.getStandardError()


def best_of_call_mc(brownian_motion, initial_values, risk_free_rate, dividend_yield, volatility, maturity, strike):
    """Value of a European call on the best of A assets, max_i S_i(T) − K floored at 0, under Black–Scholes: independent assets, asset i driven
    by factor i of `brownian_motion` (log-Euler, exact for ln S), all with one dividend yield and one volatility; `maturity` is a point of
    the time discretisation.  The maximum per path is cross_section.max_across, ONE launch for any number of assets up to 32 (the composed
    floor chain records A − 1 ops), and argmax_across says which asset it is.  Returns (value, standard error, [the fraction of paths on
    which asset i is the best performer for i]).  bermudan_max_call_mc(ordered_states=True) with the one exercise date `maturity` gives
    the same value to the last bit."""
    from .cross_section import argmax_across, max_across
    assets = len(initial_values)
    if assets < 1 or assets > brownian_motion.getNumberOfFactors(): raise ValueError("one factor of the Brownian motion per asset")
    td = brownian_motion.getTimeDiscretization()
    xs = [brownian_motion.getRandomVariableForConstant(math.log(float(s0))) for s0 in initial_values]
    drift = risk_free_rate - dividend_yield - 0.5 * volatility * volatility
    t, i = td.getTime(0), 0
    while t < maturity - 1e-12:
        xs = [x.add(drift * td.getTimeStep(i)).addProduct(brownian_motion.getBrownianIncrement(i, a), volatility) for a, x in enumerate(xs)]
        i += 1
        t = td.getTime(i)
    if abs(t - maturity) > 1e-12: raise ValueError("the maturity is not a point of the time discretisation")
    s = [x.exp() for x in xs]
    value = max_across(s).sub(strike).floor(0.0).div(math.exp(risk_free_rate * maturity))
    best = argmax_across(s)
    # asset i is the best where the index equals i: (best − i)² is 0 there and at least 1 elsewhere
    shares = [best.sub(float(a)).squared().cap(1.0).mult(-1.0).add(1.0).getAverage() for a in range(assets)]
    return value.getAverage(), value.getStandardError(), shares


def _filter_resample(weights, state, generator, scheme):
    """One resampling step of the filters below: (the resampled state, the total weight).  The systematic offset, or the m uniforms of the
    other schemes, come from `generator` on the host; nothing but the total leaves the device."""
    from .resample import resample
    if scheme == "systematic":
        (state,), total = resample(weights, [state], scheme=scheme, offset=generator.random())
    else:
        import numpy as np
        (state,), total = resample(weights, [state], scheme=scheme, uniforms=type(state)(state.getFiltrationTime(), generator.random(state.size()).astype(np.float32)))
    return state, total


def particle_filter_log_likelihood(observations, a, q, r, p0, brownian_motion, offsets_seed, scheme="systematic"):
    """log p(y_1 … y_T) of the linear-Gaussian model x_t = a·x_{t-1} + √q·ε_t, y_t = x_t + √r·η_t, x_0 ~ N(0, p0) by the BOOTSTRAP particle
    filter, one particle per path of `brownian_motion`: factor 0 of increment 0 (scaled to unit variance) draws x_0, increment t propagates
    to x_t, so the time discretisation has at least T + 1 steps.  Per observation: propagate; weight with the observation density,
    w = φ((x_t − y_t)/√r) (analytic.function_apply, NORMAL_DENSITY); add log(total/n) − log(r)/2 to the log-likelihood, total being the
    sum of the weights that the resample call returns; resample the state (resample.resample).  Nothing but `total` leaves
    the device.  The systematic offsets (one per observation; the m uniforms of the other schemes) come from a seeded HOST generator,
    numpy.random.Generator(numpy.random.PCG64(offsets_seed)).  exp of the result is an unbiased estimate of the likelihood; its logarithm is
    biased low.  A weight total of zero gives -inf.  FMHIP_DEVICE_RESAMPLE=0 gives the same number to the last bit."""
    import numpy as np
    from .analytic import NORMAL_DENSITY, function_apply
    generator = np.random.Generator(np.random.PCG64(int(offsets_seed)))
    td = brownian_motion.getTimeDiscretization()
    n = brownian_motion.getNumberOfPaths()
    x = brownian_motion.getBrownianIncrement(0, 0).mult(math.sqrt(p0 / td.getTimeStep(0)))
    log_likelihood = 0.0
    for t, y in enumerate(observations, start=1):
        x = x.mult(a).addProduct(brownian_motion.getBrownianIncrement(t, 0), math.sqrt(q / td.getTimeStep(t)))
        weights, = function_apply(x.sub(float(y)).div(math.sqrt(r)), [NORMAL_DENSITY])
        x, total = _filter_resample(weights, x, generator, scheme)
        if not total > 0.0: return -math.inf
        log_likelihood += math.log(total / n) - 0.5 * math.log(r)
    return log_likelihood


def kalman_log_likelihood(observations, a, q, r, p0):
    """The exact log p(y_1 … y_T) of particle_filter_log_likelihood's model: the Kalman filter's prediction-error decomposition, on the host."""
    mean, variance, log_likelihood = 0.0, float(p0), 0.0
    for y in observations:
        mean, variance = a * mean, a * a * variance + q
        s = variance + r
        log_likelihood += -0.5 * (math.log(2.0 * math.pi * s) + (y - mean) ** 2 / s)
        gain = variance / s
        mean, variance = mean + gain * (y - mean), (1.0 - gain) * variance
    return log_likelihood


def stochastic_volatility_log_likelihood(returns, mu, phi, sigma_eta, brownian_motion, offsets_seed, scheme="systematic"):
    """log p(y_1 … y_T) of the standard discrete stochastic-volatility model h_t = μ + φ(h_{t-1} − μ) + σ_η·η_t, y_t = exp(h_t/2)·ε_t,
    h_0 ~ N(μ, σ_η²/(1 − φ²)) (|φ| < 1), by particle_filter_log_likelihood's filter: the weight of a particle is the density of the return
    given its log-variance, φ(y_t·e^{−h_t/2})·e^{−h_t/2}.  Nothing closed-form checks it — it is the workload the resampling is for;
    FMHIP_DEVICE_RESAMPLE=0 gives the same number to the last bit.  Increments, offsets and schemes as in particle_filter_log_likelihood."""
    import numpy as np
    from .analytic import NORMAL_DENSITY, function_apply
    if not abs(phi) < 1.0: raise ValueError("the log-variance is stationary: |phi| < 1")
    generator = np.random.Generator(np.random.PCG64(int(offsets_seed)))
    td = brownian_motion.getTimeDiscretization()
    n = brownian_motion.getNumberOfPaths()
    h = brownian_motion.getBrownianIncrement(0, 0).mult(sigma_eta / math.sqrt((1.0 - phi * phi) * td.getTimeStep(0))).add(mu)
    log_likelihood = 0.0
    for t, y in enumerate(returns, start=1):
        h = h.sub(mu).mult(phi).add(mu).addProduct(brownian_motion.getBrownianIncrement(t, 0), sigma_eta / math.sqrt(td.getTimeStep(t)))
        scale = h.mult(-0.5).exp()
        density, = function_apply(scale.mult(float(y)), [NORMAL_DENSITY])
        h, total = _filter_resample(scale.mult(type(scale)(scale.getFiltrationTime(), density)), h, generator, scheme)
        if not total > 0.0: return -math.inf
        log_likelihood += math.log(total / n)
    return log_likelihood
