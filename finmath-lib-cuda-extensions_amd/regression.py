"""Least-squares regression on the device: the cross moments of many vectors in one pass (include/fmhip.h: fmhip_cross_moments, DESIGN.md
§4.8), a pivoted Cholesky of the normal equations on the host, and the conditional-expectation estimator finmath-lib's American
Monte-Carlo, Bermudan and exposure code is written against (net.finmath.montecarlo.conditionalexpectation.
MonteCarloConditionalExpectationRegression).

finmath-lib assembles XᵀX and Xᵀy as b_i.mult(b_j).getAverage(): one recorded product and one blocking expectation per pair, every basis
vector read about K times.  Here the K + 1 vectors are read once and the K(K+1)/2 + K sums come out of one launch.  The estimator is
written against the RandomVariable interface and accepts any factory's vectors: the one-pass path is taken when every stochastic operand
is a RandomVariableHip, the product-by-product path otherwise (and with FMHIP_DEVICE_CROSS_MOMENTS=0: the A/B switch and the fallback).

Wide regression: more than 12 + 4 vectors, up to 64 in all, go to fmhip_cross_moments_wide — the same sums from one
pass on the matrix cores —, so the estimator keeps its one-pass path up to 60 basis functions (a Longstaff–Schwartz basis on several
underlyings) and covariance_matrix takes 63 vectors.  FMHIP_DEVICE_WIDE_MOMENTS=0: the estimator goes pair by pair beyond 12 basis
functions, as it did before the wide pass existed.

Localized regression: a global polynomial is the wrong tool for a kinked continuation value.  binned_cross_moments
returns the cross moments PER BIN of a key vector from one launch (fmhip_binned_cross_moments) — the block-diagonal normal equations of a
fit that is local in the key —, quantile_bounds the bounds of bins of equal count, binned_evaluate the piecewise estimate as a new vector,
and MonteCarloConditionalExpectationLocalizedRegression the estimator on top of them (finmath-lib: BermudanOption's binning basis, the
…LocalizedOnDependentRegression factories).  FMHIP_DEVICE_BINNED_MOMENTS=0 or any other RandomVariable class: indicators by choose and
averages pair by pair.

Polynomial regression in one pass: a polynomial basis need not exist in memory.  polynomial_cross_moments returns the
sums — and the bits — the wide pass returns for the materialised monomials, from the state vectors and an exponent table
(fmhip_polynomial_cross_moments: the monomials are formed in registers), polynomial_evaluate the fitted polynomial as a new vector, and
MonteCarloConditionalExpectationPolynomialRegression the estimator on top of them.  FMHIP_DEVICE_POLYNOMIAL_MOMENTS=0: the monomials are
materialised by mult chains and MonteCarloConditionalExpectationRegression does the rest, as before the pass existed."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip, select_ranks_batch

MAX_X, MAX_Y = 12, 4                     # fmhip_cross_moments' limits
WIDE_MAX = 64                            # fmhip_cross_moments_wide's limit: x and y together
WIDE_MAX_BASIS = 60                      # the estimator's one-pass path: at least four dependents per call
BINNED_MAX_X, BINNED_MAX_Y, MAX_BINS = 3, 4, 64      # fmhip_binned_cross_moments' limits
POLY_MAX_STATES, POLY_MAX_EXPONENT = 8, 6            # fmhip_polynomial_cross_moments' limits
PIVOT_TOLERANCE = 1e-12                  # a basis function whose remaining pivot is <= this x the largest diagonal entry is dropped


def device_cross_moments() -> bool:
    """FMHIP_DEVICE_CROSS_MOMENTS=0: the estimator builds the normal equations product by product, as finmath-lib does; anything else:
    one fmhip_cross_moments call."""
    return os.environ.get("FMHIP_DEVICE_CROSS_MOMENTS", "1") != "0"


def device_wide_moments() -> bool:
    """FMHIP_DEVICE_WIDE_MOMENTS=0: beyond 12 basis functions the estimator builds the normal equations product by product (the A/B
    switch and the fallback); anything else: fmhip_cross_moments_wide, one call per 64 − K dependents.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_WIDE_MOMENTS", "1") != "0"


def _handle(v, allow_one: bool) -> int:
    if v is None or (np.isscalar(v) and float(v) == 1.0):
        if not allow_one: raise ValueError("the constant 1 is an x, not a y")
        return 0
    if isinstance(v, RandomVariableHip):
        if v.isDeterministic(): raise ValueError("a deterministic random variable has no vector: fold its value on the host (pass None for the constant 1)")
        v = v.realizations
    return int(getattr(v, "handle", v))


def cross_moments(xs, ys=()):
    """(S, T): S[i][j] = Σ_p x_i[p]·x_j[p] (full symmetric n_x × n_x), T[i][m] = Σ_p x_i[p]·y_m[p] (n_x × n_y), fp64 SUMS from one device
    launch.  Entries: RandomVariableHip, DeviceVector or raw handles; an x may be None or 1.0 for the constant 1, which then also yields
    the plain sums Σ x_j and, at (ones, ones), n.  Up to 12 xs and 4 ys go to fmhip_cross_moments (and keep its bits); anything larger, up
    to 64 vectors in all, goes to fmhip_cross_moments_wide."""
    xs, ys = list(xs), list(ys)
    nx, ny = len(xs), len(ys)
    wide = nx > MAX_X or ny > MAX_Y
    if wide and nx + ny > WIDE_MAX: raise ValueError(f"cross moments of {nx} + {ny} vectors: at most {WIDE_MAX} in one call")
    hx = (C.c_int64 * max(nx, 1))(*[_handle(v, True) for v in xs])
    hy = (C.c_int64 * max(ny, 1))(*[_handle(v, False) for v in ys])
    out = np.empty(nx * (nx + 1) // 2 + nx * ny, dtype=np.float64)
    call = N.lib().fmhip_cross_moments_wide if wide else N.lib().fmhip_cross_moments
    N.check(call(hx, nx, hy if ny else None, ny, out.ctypes.data_as(C.POINTER(C.c_double))))
    S = np.empty((nx, nx), dtype=np.float64)
    iu = np.triu_indices(nx)
    S[iu] = out[:iu[0].size]
    S.T[iu] = out[:iu[0].size]
    return S, out[iu[0].size:].reshape(nx, ny).copy()


def covariance_matrix(vectors) -> np.ndarray:
    """Population covariance of up to 63 vectors (up to 11: the narrow pass and its bits) from ONE pass: S_ij/n − mean_i·mean_j in fp64, with the means and n from the ones entry.
    The subtraction cancels: the result carries an absolute error of about 2⁻⁵³·(|S_ij|/n + |mean_i·mean_j|)·log2(n), which is all of it
    when the standard deviations are below ~1e-8 of the means — shift such data first."""
    vectors = list(vectors)
    S, _ = cross_moments([None] + vectors)
    n = S[0, 0]
    mean = S[0, 1:] / n
    return S[1:, 1:] / n - np.outer(mean, mean)


def solve_normal_equations(A, b) -> np.ndarray:
    """x with A x = b in the least-squares sense for a symmetric positive SEMI-definite A (K × K; b: K or K × M): Cholesky with diagonal
    pivoting in fp64.  The largest remaining pivot is taken next (the first of equals); once it is <= 1e-12 × the largest diagonal entry of
    A, the remaining unknowns are 0 — a collinear basis function, the indicator of an empty bin.  The C++ and Java mirrors implement the
    same rule step for step, so their coefficients agree to rounding."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(b, dtype=np.float64)
    one = B.ndim == 1
    B = B.reshape(A.shape[0], -1)
    K = A.shape[0]
    if K > MAX_X:                        # the loops below are cubic in K in the interpreter: ~100 µs at K = 12, more than the pass at K = 56
        x = _solve_normal_equations_rows(A, B)
        return x[:, 0] if one else x
    perm = list(range(K))
    d = [float(A[i, i]) for i in range(K)]
    tol = PIVOT_TOLERANCE * max(d) if K else 0.0
    L = np.zeros((K, K))                 # row = unknown, column = elimination step
    rank = K
    for k in range(K):
        p = k
        for q in range(k + 1, K):
            if d[perm[q]] > d[perm[p]]: p = q
        if d[perm[p]] <= tol:
            rank = k
            break
        perm[k], perm[p] = perm[p], perm[k]
        i = perm[k]
        L[i, k] = math.sqrt(d[i])
        for q in range(k + 1, K):
            j = perm[q]
            s = float(A[j, i])
            for t in range(k): s -= L[j, t] * L[i, t]
            L[j, k] = s / L[i, k]
            d[j] -= L[j, k] * L[j, k]
    x = np.zeros((K, B.shape[1]))
    for m in range(B.shape[1]):
        z = [0.0] * rank
        for k in range(rank):            # L z = b
            s = float(B[perm[k], m])
            for t in range(k): s -= L[perm[k], t] * z[t]
            z[k] = s / L[perm[k], k]
        for k in range(rank - 1, -1, -1):            # Lᵀ x = z
            s = z[k]
            for t in range(k + 1, rank): s -= L[perm[t], k] * x[perm[t], m]
            x[perm[k], m] = s / L[perm[k], k]
    return x[:, 0] if one else x


def _solve_normal_equations_rows(A, B) -> np.ndarray:
    """solve_normal_equations for K > 12: the same algorithm — the same diagonal pivoting (the first of equals), the same 1e-12 rule — with
    every loop over the remaining unknowns as one numpy row operation."""
    K = A.shape[0]
    perm = np.arange(K)
    d = A.diagonal().copy()
    tol = PIVOT_TOLERANCE * d.max()
    L = np.zeros((K, K))                 # row = unknown, column = elimination step
    rank = K
    for k in range(K):
        p = k + int(np.argmax(d[perm[k:]]))
        if not d[perm[p]] > tol:
            rank = k
            break
        perm[[k, p]] = perm[[p, k]]
        i, rest = perm[k], perm[k + 1:]
        L[i, k] = math.sqrt(d[i])
        L[rest, k] = (A[rest, i] - L[rest, :k] @ L[i, :k]) / L[i, k]
        d[rest] -= L[rest, k] * L[rest, k]
    kept = perm[:rank]
    Lp = L[kept, :rank]                  # lower triangular in elimination order
    z = np.zeros((rank, B.shape[1]))
    for k in range(rank):                # L z = b
        z[k] = (B[kept[k]] - Lp[k, :k] @ z[:k]) / Lp[k, k]
    for k in range(rank - 1, -1, -1):    # Lᵀ x = z, in place
        z[k] = (z[k] - Lp[k + 1:, k] @ z[k + 1:]) / Lp[k, k]
    x = np.zeros((K, B.shape[1]))
    x[kept] = z
    return x


class MonteCarloConditionalExpectationRegression:
    """E[ · | basis functions] by least squares (finmath-lib: MonteCarloConditionalExpectationRegression).  `basisFunctionsEstimator`
    are the regressors the parameters are estimated on, `basisFunctionsPredictor` (default: the same) the ones the estimate is evaluated
    on.  Any RandomVariable implementation is accepted."""

    def __init__(self, basisFunctionsEstimator, basisFunctionsPredictor=None):
        self.basisFunctionsEstimator = list(basisFunctionsEstimator)
        self.basisFunctionsPredictor = list(basisFunctionsPredictor) if basisFunctionsPredictor is not None else self.basisFunctionsEstimator
        if len(self.basisFunctionsPredictor) != len(self.basisFunctionsEstimator):
            raise ValueError("estimator and predictor need the same number of basis functions")

    # ---- the normal equations, as averages
    def _one_pass(self, dependents) -> bool:
        basis = self.basisFunctionsEstimator
        if not device_cross_moments() or not 1 <= len(basis) <= WIDE_MAX_BASIS or not dependents: return False
        if len(basis) > MAX_X and not device_wide_moments(): return False
        if not all(isinstance(v, RandomVariableHip) for v in basis + dependents): return False
        # the constant 1 stands in for deterministic basis functions; dependents and at least one basis function must be vectors
        return all(not y.isDeterministic() for y in dependents) and any(not b.isDeterministic() for b in basis)

    def _normal_equations_device(self, dependents):
        basis = self.basisFunctionsEstimator
        scale = np.array([b.doubleValue() if b.isDeterministic() else 1.0 for b in basis])      # c·Σx_j, c·c'·n through the ones entry
        xs = [None if b.isDeterministic() else b for b in basis]
        n = float(next(b for b in basis if not b.isDeterministic())._sample_size())
        A, cols = None, []
        step = MAX_Y if len(basis) <= MAX_X else WIDE_MAX - len(basis)      # beyond 12 basis functions: the wide pass, 64 − K dependents a call
        for m0 in range(0, len(dependents), step):
            S, T = cross_moments(xs, dependents[m0:m0 + step])
            A = S
            cols.append(T)
        return A * np.outer(scale, scale) / n, np.hstack(cols) * scale[:, None] / n

    def _normal_equations_generic(self, dependents):
        basis = self.basisFunctionsEstimator
        K = len(basis)
        A = np.empty((K, K))
        for i in range(K):
            for j in range(i, K):
                A[i, j] = A[j, i] = basis[i].mult(basis[j]).getAverage()
        b = np.array([[basis[i].mult(y).getAverage() for y in dependents] for i in range(K)], dtype=np.float64).reshape(K, len(dependents))
        return A, b

    def getLinearRegressionParameters(self, dependents) -> np.ndarray:
        """β (K) for one dependent, K × M for a sequence of M dependents (one pass per four of them; per 64 − K beyond 12 basis
        functions)."""
        one = not isinstance(dependents, (list, tuple))
        ys = [dependents] if one else list(dependents)
        A, b = self._normal_equations_device(ys) if self._one_pass(ys) else self._normal_equations_generic(ys)
        beta = solve_normal_equations(A, b)
        return beta[:, 0] if one else beta

    def getConditionalExpectation(self, dependents):
        """Σ β_i·b_i over the predictor's basis functions, built with mult / addProduct as finmath-lib builds it (one fused chain on the
        engine)."""
        beta = self.getLinearRegressionParameters(dependents)
        one = beta.ndim == 1
        beta = beta.reshape(len(self.basisFunctionsPredictor), -1)
        out = []
        for m in range(beta.shape[1]):
            basis = self.basisFunctionsPredictor
            ce = basis[0].mult(float(beta[0, m]))
            for i in range(1, len(basis)):
                ce = ce.addProduct(basis[i], float(beta[i, m]))
            out.append(ce)
        return out[0] if one else out


# ------------------------------------------------------------------ localized regression
def device_binned_moments() -> bool:
    """FMHIP_DEVICE_BINNED_MOMENTS=0: the localized estimator builds indicators by choose and averages pair by pair (the A/B switch and the
    fallback); anything else: one fmhip_binned_cross_moments call per four dependents and one fmhip_binned_evaluate call per estimate."""
    return os.environ.get("FMHIP_DEVICE_BINNED_MOMENTS", "1") != "0"


def _bounds(bounds):
    b = np.ascontiguousarray(bounds, dtype=np.float64).ravel()
    return b, (b.ctypes.data_as(C.POINTER(C.c_double)) if b.size else None)


def binned_cross_moments(key, bounds, xs, ys=()):
    """(counts, S, T) per bin of `key`, bin(k) = #{ j : bounds[j] < k } (len(bounds) + 1 bins, at most 64): counts[b] paths (int64),
    S[b] = Σ x_i·x_j (full symmetric n_x × n_x) and T[b] = Σ x_i·y_m (n_x × n_y) over the paths of bin b, fp64 SUMS from one device launch.
    At most 3 xs (None or 1.0: the constant 1) and 4 ys."""
    xs, ys = list(xs), list(ys)
    nx, ny = len(xs), len(ys)
    b, pb = _bounds(bounds)
    n_bins = b.size + 1
    hx = (C.c_int64 * max(nx, 1))(*[_handle(v, True) for v in xs])
    hy = (C.c_int64 * max(ny, 1))(*[_handle(v, False) for v in ys])
    q = nx * (nx + 1) // 2 + nx * ny
    counts = np.zeros(n_bins, dtype=np.int64)
    out = np.empty(max(n_bins, 1) * q, dtype=np.float64)
    N.check(N.lib().fmhip_binned_cross_moments(_handle(key, False), pb, n_bins, hx, nx, hy if ny else None, ny,
                                               counts.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_double))))
    out = out.reshape(n_bins, q)
    S = np.empty((n_bins, nx, nx), dtype=np.float64)
    iu = np.triu_indices(nx)
    S[:, iu[0], iu[1]] = out[:, :iu[0].size]
    S[:, iu[1], iu[0]] = out[:, :iu[0].size]
    return counts, S, out[:, iu[0].size:].reshape(n_bins, nx, ny).copy()


def binned_evaluate(key, bounds, xs, coefficients) -> DeviceVector:
    """The piecewise estimate as a new device vector: ((x_0·c_0) + x_1·c_1) + x_2·c_2 with c = (float)coefficients[bin(key)], every fp32
    operation rounded on its own (fmhip_binned_evaluate).  coefficients: (len(bounds) + 1) × len(xs)."""
    xs = list(xs)
    b, pb = _bounds(bounds)
    c = np.ascontiguousarray(coefficients, dtype=np.float64).reshape(b.size + 1, len(xs))
    hx = (C.c_int64 * max(len(xs), 1))(*[_handle(v, True) for v in xs])
    out = C.c_int64(0)
    N.check(N.lib().fmhip_binned_evaluate(_handle(key, False), pb, b.size + 1, hx, len(xs), c.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out)))
    k = key.realizations if isinstance(key, RandomVariableHip) else key
    return DeviceVector(out.value, k.n)


def quantile_rank(j: int, n: int, n_bins: int) -> int:
    """Rank (0-based, ascending) of the upper bound of bin j - 1 of n_bins bins of equal count: ceil(j·n / n_bins) − 1."""
    return max((j * n + n_bins - 1) // n_bins - 1, 0)


def quantile_bounds(key, n_bins: int) -> np.ndarray:
    """Bounds of n_bins bins of (nearly) equal count: sorted(key)[ceil(j·n/n_bins) − 1] for j = 1 … n_bins − 1 — elements of the vector,
    taken by ONE select_ranks_batch call on the device (n: the sample behind the expectation communicator, if one is set); a host sort for
    any other RandomVariable class."""
    if isinstance(key, (RandomVariableHip, DeviceVector)):
        v = key.realizations if isinstance(key, RandomVariableHip) else key
        w = C.c_int(1)
        N.check(N.lib().fmhip_expectation_world(C.byref(w), None))
        n = v.n * w.value
        if n_bins <= 1: return np.empty(0, dtype=np.float64)
        return select_ranks_batch([v], [quantile_rank(j, n, n_bins) for j in range(1, n_bins)])[0]
    a = np.sort(np.asarray(key.getRealizations(), dtype=np.float64))
    return np.array([a[quantile_rank(j, a.size, n_bins)] for j in range(1, n_bins)], dtype=np.float64)


class MonteCarloConditionalExpectationLocalizedRegression:
    """E[ · | key, basis functions] by a least-squares fit PER BIN of `key` (finmath-lib: the binning basis of BermudanOption, the
    …LocalizedOnDependentRegression estimators): n_bins bins, bounded by `bounds` (n_bins − 1 ascending values; default: quantile_bounds, bins
    of equal count), bin(k) = #{ j : bounds[j] < k }.  The normal equations are block diagonal — one K × K block per bin, solved by
    solve_normal_equations, so an empty bin gets coefficients 0.  Written against the RandomVariable interface; the device path (one
    fmhip_binned_cross_moments call, one fmhip_binned_evaluate call) is taken when every stochastic operand is a RandomVariableHip and
    K <= 3, the generic path (indicators by choose, averages pair by pair) otherwise and with FMHIP_DEVICE_BINNED_MOMENTS=0.  The generic
    path compares in the key class's own arithmetic: it agrees with the device path (NaN and infinite keys included) for bounds that are
    fp32 values — quantile bounds are elements of the key — and deviates for bounds that are not, and for a key of −inf against a bound of
    −inf (see _triggers)."""

    def __init__(self, key, n_bins, basisFunctionsEstimator, basisFunctionsPredictor=None, bounds=None):
        if not 1 <= int(n_bins) <= MAX_BINS: raise ValueError(f"n_bins must be 1 … {MAX_BINS}")
        if key.isDeterministic(): raise ValueError("the key of a localized regression is a stochastic random variable")
        self.key, self.n_bins = key, int(n_bins)
        self.basisFunctionsEstimator = list(basisFunctionsEstimator)
        self.basisFunctionsPredictor = list(basisFunctionsPredictor) if basisFunctionsPredictor is not None else self.basisFunctionsEstimator
        if len(self.basisFunctionsPredictor) != len(self.basisFunctionsEstimator):
            raise ValueError("estimator and predictor need the same number of basis functions")
        self.bounds = np.asarray(bounds, dtype=np.float64).ravel() if bounds is not None else quantile_bounds(key, self.n_bins)
        if self.bounds.size != self.n_bins - 1: raise ValueError("n_bins bins have n_bins − 1 bounds")
        if np.isnan(self.bounds).any() or (np.diff(self.bounds) < 0).any(): raise ValueError("the bounds are ascending and not NaN")
        self._indicators = None

    # ---- which path
    def _device(self, basis, others) -> bool:
        if not device_binned_moments() or not 1 <= len(basis) <= BINNED_MAX_X: return False
        if not all(isinstance(v, RandomVariableHip) for v in [self.key] + basis + others): return False
        return all(not y.isDeterministic() for y in others)

    # ---- generic path: the bins from the RandomVariable interface.  Membership is decided by the trigger bound − key >= 0 (⟺ key <= bound) in
    # the arithmetic of the key's class.  NaN keys are taken out with isNaN (no bin; the estimate is NaN there), and an infinite bound is not
    # subtracted (inf − inf is NaN): nothing is above +inf, everything is above −inf.  What still deviates from the device path: a bound that
    # is not an fp32 value is rounded to one by an fp32 class before it is compared, and a key of −inf against a bound of −inf counts as
    # above it.  Quantile bounds of finite keys produce neither.
    def _zero(self):
        return self.key.isNaN().mult(0.0)                              # 0 on every path, whatever the key holds

    def _triggers(self):
        return [self._zero().add(1.0 if b > 0 else -1.0) if math.isinf(b) else self.key.bus(float(b)) for b in self.bounds]

    def _bin_indicators(self):
        if self._indicators is None:
            zero = self._zero()
            one = zero.add(1.0)
            valid = one.sub(self.key.isNaN())
            below = [t.choose(valid, zero) for t in self._triggers()] + [valid]      # 1 where key <= bounds[b]; the last bin takes the rest
            self._indicators = [below[0]] + [below[b].sub(below[b - 1]) for b in range(1, self.n_bins)]
        return self._indicators

    def _normal_equations_generic(self, dependents):
        basis, K = self.basisFunctionsEstimator, len(self.basisFunctionsEstimator)
        A = np.empty((self.n_bins, K, K)); T = np.empty((self.n_bins, K, len(dependents)))
        zero = self._zero()
        for b, ind in enumerate(self._bin_indicators()):
            member = ind.sub(0.5)
            local = [member.choose(f, zero) if not f.isDeterministic() else ind.mult(f.doubleValue()) for f in basis]      # SELECTED, not multiplied: a NaN outside the bin stays outside
            for i in range(K):
                for j in range(i, K):
                    A[b, i, j] = A[b, j, i] = local[i].mult(local[j]).getAverage()
                for m, y in enumerate(dependents):
                    T[b, i, m] = local[i].mult(member.choose(y, zero)).getAverage()
        return A, T

    def _normal_equations_device(self, dependents):
        basis = self.basisFunctionsEstimator
        scale = np.array([f.doubleValue() if f.isDeterministic() else 1.0 for f in basis])
        xs = [None if f.isDeterministic() else f for f in basis]
        n = float(self.key._sample_size())
        A, cols = None, []
        for m0 in range(0, len(dependents), BINNED_MAX_Y):
            _, S, T = binned_cross_moments(self.key, self.bounds, xs, dependents[m0:m0 + BINNED_MAX_Y])
            A = S
            cols.append(T)
        return A * np.outer(scale, scale)[None] / n, np.concatenate(cols, axis=2) * scale[None, :, None] / n

    def getBinCounts(self) -> np.ndarray:
        """Paths per bin (of the global sample behind an expectation communicator)."""
        if device_binned_moments() and isinstance(self.key, RandomVariableHip):
            return binned_cross_moments(self.key, self.bounds, [None])[0]
        n = self.key.size()
        return np.array([int(round(ind.getAverage() * n)) for ind in self._bin_indicators()], dtype=np.int64)

    def getLinearRegressionParameters(self, dependents) -> np.ndarray:
        """β: n_bins × K for one dependent, n_bins × K × M for a sequence of M dependents (one pass per four of them)."""
        one = not isinstance(dependents, (list, tuple))
        ys = [dependents] if one else list(dependents)
        A, T = self._normal_equations_device(ys) if self._device(self.basisFunctionsEstimator, ys) else self._normal_equations_generic(ys)
        beta = np.stack([solve_normal_equations(A[b], T[b]) for b in range(self.n_bins)])
        return beta[:, :, 0] if one else beta

    def _evaluate(self, beta):
        basis = self.basisFunctionsPredictor
        if self._device(basis, []) and all((not f.isDeterministic()) or f.doubleValue() == 1.0 for f in basis) and any(not f.isDeterministic() for f in basis + [self.key]):
            xs = [None if f.isDeterministic() else f for f in basis]
            time = max([self.key.getFiltrationTime()] + [f.getFiltrationTime() for f in basis])
            return RandomVariableHip(time, binned_evaluate(self.key, self.bounds, xs, beta))
        chains = []
        for b in range(self.n_bins):
            ce = basis[0].mult(float(beta[b, 0]))
            for i in range(1, len(basis)): ce = ce.addProduct(basis[i], float(beta[b, i]))
            chains.append(ce)
        zero = self._zero()
        as_vector = lambda c: c if not c.isDeterministic() else zero.add(c.doubleValue())
        out = as_vector(chains[-1])
        for b, t in reversed(list(enumerate(self._triggers()))):
            out = t.choose(as_vector(chains[b]), out)
        return self.key.isNaN().sub(0.5).choose(zero.add(math.nan), out)      # a NaN key has no bin

    def getConditionalExpectation(self, dependents):
        """Per path the fit of its bin: Σ β[bin]_i·b_i over the predictor's basis functions, in the fp32 arithmetic of
        basis[0].mult(β0).addProduct(basis[i], βi)."""
        beta = self.getLinearRegressionParameters(dependents)
        if beta.ndim == 2: return self._evaluate(beta)
        return [self._evaluate(beta[:, :, m]) for m in range(beta.shape[2])]


# ------------------------------------------------------------------ polynomial regression in one pass
def device_polynomial_moments() -> bool:
    """FMHIP_DEVICE_POLYNOMIAL_MOMENTS=0: the polynomial estimator materialises its monomials by mult chains and hands them to
    MonteCarloConditionalExpectationRegression (the A/B switch and the fallback: exactly the code path there was before); anything else:
    fmhip_polynomial_cross_moments and fmhip_polynomial_evaluate on the state vectors.  Read per call."""
    return os.environ.get("FMHIP_DEVICE_POLYNOMIAL_MOMENTS", "1") != "0"


def _exponent_table(exponents, n_states):
    e = np.ascontiguousarray(exponents, dtype=np.int64).reshape(-1, n_states)
    if e.size == 0: raise ValueError("a polynomial basis has at least one term")
    if e.min() < 0 or e.max() > 255: raise ValueError("exponents are 0 … 6")
    e = np.ascontiguousarray(e, dtype=np.uint8)
    return e, e.ctypes.data_as(C.POINTER(C.c_uint8))


def polynomial_cross_moments(states, exponents, extra=(), ys=()):
    """(S, T) of cross_moments for the regressors [monomials of `states` by the rows of `exponents`…, extra…] and the dependents ys, from
    the STATE vectors: the monomials are formed in registers (fmhip_polynomial_cross_moments), never stored.  The sums are, bit for bit, the
    wide pass's for the same list with the monomials materialised by monomial_basis' mult chains.  At most 8 states, exponents 0 … 6 (a
    row of zeros: the constant 1), len(exponents) + len(extra) + len(ys) <= 64; an extra may be None or 1.0 for the constant 1."""
    states, extra, ys = list(states), list(extra), list(ys)
    e, pe = _exponent_table(exponents, len(states))
    nt, ne, ny = e.shape[0], len(extra), len(ys)
    nx = nt + ne
    hs = (C.c_int64 * max(len(states), 1))(*[_handle(v, False) for v in states])
    hx = (C.c_int64 * max(ne, 1))(*[_handle(v, True) for v in extra])
    hy = (C.c_int64 * max(ny, 1))(*[_handle(v, False) for v in ys])
    out = np.empty(nx * (nx + 1) // 2 + nx * ny, dtype=np.float64)
    N.check(N.lib().fmhip_polynomial_cross_moments(hs, len(states), pe, nt, hx if ne else None, ne, hy if ny else None, ny, out.ctypes.data_as(C.POINTER(C.c_double))))
    S = np.empty((nx, nx), dtype=np.float64)
    iu = np.triu_indices(nx)
    S[iu] = out[:iu[0].size]
    S.T[iu] = out[:iu[0].size]
    return S, out[iu[0].size:].reshape(nx, ny).copy()


def polynomial_evaluate(states, exponents, coefficients, extra=()) -> DeviceVector:
    """The fitted polynomial as a new device vector: ((t_0·c_0) + t_1·c_1) + … over the monomials, then the extras, c = (float)coefficients,
    every fp32 operation rounded on its own (fmhip_polynomial_evaluate) — the bits of basis[0].mult(c0).addProduct(basis[1], c1)… on the
    materialised basis."""
    states, extra = list(states), list(extra)
    e, pe = _exponent_table(exponents, len(states))
    c = np.ascontiguousarray(coefficients, dtype=np.float64).ravel()
    if c.size != e.shape[0] + len(extra): raise ValueError("one coefficient per term and per extra vector")
    hs = (C.c_int64 * max(len(states), 1))(*[_handle(v, False) for v in states])
    hx = (C.c_int64 * max(len(extra), 1))(*[_handle(v, True) for v in extra])
    out = C.c_int64(0)
    N.check(N.lib().fmhip_polynomial_evaluate(hs, len(states), pe, e.shape[0], hx if extra else None, len(extra), c.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out)))
    first = states[0].realizations if isinstance(states[0], RandomVariableHip) else states[0]
    return DeviceVector(out.value, first.n)


def monomial_basis(states, exponents, one=None):
    """The monomials of `states` as random variables, by the chain that is the contract of the one-pass path: powers u, u·u, (u·u)·u … by
    mult, a monomial the product of its non-trivial powers in ascending state index, left to right.  A row of zeros is `one` (default: the
    deterministic 1 of the first state's class, built as cls(time, value))."""
    states = list(states)
    rows = [tuple(int(x) for x in row) for row in np.asarray(exponents, dtype=np.int64).reshape(-1, len(states))]
    top = max((max(r) for r in rows), default=0)
    if one is None: one = type(states[0])(-math.inf, 1.0)
    powers = [[one, u] for u in states]
    for p in powers:
        for _ in range(2, top + 1): p.append(p[-1].mult(p[1]))
    basis = []
    for row in rows:
        f = None
        for a, ea in enumerate(row):
            if ea: f = powers[a][ea] if f is None else f.mult(powers[a][ea])
        basis.append(one if f is None else f)
    return basis


class MonteCarloConditionalExpectationPolynomialRegression:
    """E[ · | polynomial in the states] by least squares, the basis given as an exponent table instead of vectors: every monomial of total
    degree <= `order` in `states` (montecarlo.monomial_exponents; or the rows of `exponents`), then `extra_basis` (ordinary regressors: an
    exercise value, a spline).  Semantics of MonteCarloConditionalExpectationRegression with estimator = predictor.  The one-pass path —
    fmhip_polynomial_cross_moments per 64 − K dependents, one fmhip_polynomial_evaluate per estimate: no monomial is ever stored — is taken
    when every state, extra and dependent is a non-deterministic RandomVariableHip, K <= 60 and FMHIP_DEVICE_POLYNOMIAL_MOMENTS is not 0;
    otherwise the monomials are materialised by monomial_basis and MonteCarloConditionalExpectationRegression does the rest.  Both paths
    agree to the last bit wherever that estimator takes the wide pass (K > 12)."""

    def __init__(self, states, order=None, exponents=None, extra_basis=(), one=None):
        """one: the constant 1 of the materialised basis, as a random variable of the states' class (default: cls(−inf, 1.0))."""
        self.states, self.one = list(states), one
        if not self.states: raise ValueError("a polynomial regression needs at least one state")
        if exponents is None:
            if order is None: raise ValueError("give the order of the polynomial or its exponents")
            from .montecarlo import monomial_exponents
            exponents = monomial_exponents(len(self.states), int(order))
        self.exponents = np.ascontiguousarray(exponents, dtype=np.int64).reshape(-1, len(self.states))
        if self.exponents.shape[0] < 1 or self.exponents.min() < 0: raise ValueError("a polynomial basis has at least one term and no negative exponent")
        self.extra_basis = list(extra_basis)
        self._materialised = None

    def _one_pass(self, dependents) -> bool:
        K = self.exponents.shape[0] + len(self.extra_basis)
        if not device_polynomial_moments() or K > WIDE_MAX_BASIS or len(self.states) > POLY_MAX_STATES or self.exponents.max() > POLY_MAX_EXPONENT: return False
        return all(isinstance(v, RandomVariableHip) and not v.isDeterministic() for v in self.states + self.extra_basis + list(dependents))

    def _generic(self):
        if self._materialised is None:
            self._materialised = MonteCarloConditionalExpectationRegression(monomial_basis(self.states, self.exponents, self.one) + self.extra_basis)
        return self._materialised

    def getLinearRegressionParameters(self, dependents) -> np.ndarray:
        """β (K) for one dependent, K × M for a sequence of M dependents (one pass per 64 − K of them)."""
        one = not isinstance(dependents, (list, tuple))
        ys = [dependents] if one else list(dependents)
        if not ys or not self._one_pass(ys): return self._generic().getLinearRegressionParameters(dependents)
        K = self.exponents.shape[0] + len(self.extra_basis)
        n = float(self.states[0]._sample_size())
        A, cols = None, []
        step = WIDE_MAX - K
        for m0 in range(0, len(ys), step):
            S, T = polynomial_cross_moments(self.states, self.exponents, self.extra_basis, ys[m0:m0 + step])
            A = S
            cols.append(T)
        scale = np.ones(K)                   # (the arithmetic of the materialised estimator, factor for factor)
        beta = solve_normal_equations(A * np.outer(scale, scale) / n, np.hstack(cols) * scale[:, None] / n)
        return beta[:, 0] if one else beta

    def getConditionalExpectation(self, dependents):
        """The fitted polynomial on the states, in the fp32 arithmetic of basis[0].mult(β0).addProduct(basis[i], βi)."""
        one = not isinstance(dependents, (list, tuple))
        ys = [dependents] if one else list(dependents)
        if not ys or not self._one_pass(ys): return self._generic().getConditionalExpectation(dependents)
        beta = self.getLinearRegressionParameters(ys)
        time = max(v.getFiltrationTime() for v in self.states + self.extra_basis)
        out = [RandomVariableHip(time, polynomial_evaluate(self.states, self.exponents, beta[:, m], self.extra_basis)) for m in range(beta.shape[1])]
        return out[0] if one else out
