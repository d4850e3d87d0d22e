"""Least-squares regression on the device: the cross moments of many vectors in one pass (include/fmhip.h: fmhip_cross_moments, DESIGN.md
§4.8), a pivoted Cholesky of the normal equations on the host, and the conditional-expectation estimator finmath-lib's American
Monte-Carlo, Bermudan and exposure code is written against (net.finmath.montecarlo.conditionalexpectation.
MonteCarloConditionalExpectationRegression).

finmath-lib assembles XᵀX and Xᵀy as b_i.mult(b_j).getAverage(): one recorded product and one blocking expectation per pair, every basis
vector read about K times.  Here the K + 1 vectors are read once and the K(K+1)/2 + K sums come out of one launch.  The estimator is
written against the RandomVariable interface and accepts any factory's vectors: the one-pass path is taken when every stochastic operand
is a RandomVariableHip, the product-by-product path otherwise (and with FMHIP_DEVICE_CROSS_MOMENTS=0: the A/B switch and the fallback)."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import _native as N
from .random_variable import DeviceVector, RandomVariableHip

MAX_X, MAX_Y = 12, 4                     # fmhip_cross_moments' limits
PIVOT_TOLERANCE = 1e-12                  # a basis function whose remaining pivot is <= this x the largest diagonal entry is dropped


def device_cross_moments() -> bool:
    """FMHIP_DEVICE_CROSS_MOMENTS=0: the estimator builds the normal equations product by product, as finmath-lib does; anything else:
    one fmhip_cross_moments call."""
    return os.environ.get("FMHIP_DEVICE_CROSS_MOMENTS", "1") != "0"


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
    the plain sums Σ x_j and, at (ones, ones), n.  At most 12 xs and 4 ys."""
    xs, ys = list(xs), list(ys)
    nx, ny = len(xs), len(ys)
    hx = (C.c_int64 * max(nx, 1))(*[_handle(v, True) for v in xs])
    hy = (C.c_int64 * max(ny, 1))(*[_handle(v, False) for v in ys])
    out = np.empty(nx * (nx + 1) // 2 + nx * ny, dtype=np.float64)
    N.check(N.lib().fmhip_cross_moments(hx, nx, hy if ny else None, ny, out.ctypes.data_as(C.POINTER(C.c_double))))
    S = np.empty((nx, nx), dtype=np.float64)
    iu = np.triu_indices(nx)
    S[iu] = out[:iu[0].size]
    S.T[iu] = out[:iu[0].size]
    return S, out[iu[0].size:].reshape(nx, ny).copy()


def covariance_matrix(vectors) -> np.ndarray:
    """Population covariance of up to 11 vectors from ONE pass: S_ij/n − mean_i·mean_j in fp64, with the means and n from the ones entry.
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
        if not device_cross_moments() or not 1 <= len(basis) <= MAX_X or not dependents: return False
        if not all(isinstance(v, RandomVariableHip) for v in basis + dependents): return False
        # the constant 1 stands in for deterministic basis functions; dependents and at least one basis function must be vectors
        return all(not y.isDeterministic() for y in dependents) and any(not b.isDeterministic() for b in basis)

    def _normal_equations_device(self, dependents):
        basis = self.basisFunctionsEstimator
        scale = np.array([b.doubleValue() if b.isDeterministic() else 1.0 for b in basis])      # c·Σx_j, c·c'·n through the ones entry
        xs = [None if b.isDeterministic() else b for b in basis]
        n = float(next(b for b in basis if not b.isDeterministic())._sample_size())
        A, cols = None, []
        for m0 in range(0, len(dependents), MAX_Y):
            S, T = cross_moments(xs, dependents[m0:m0 + MAX_Y])
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
        """β (K) for one dependent, K × M for a sequence of M dependents (one pass per four of them)."""
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
