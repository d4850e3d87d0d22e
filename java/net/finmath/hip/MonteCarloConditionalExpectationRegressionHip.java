package net.finmath.hip;

import net.finmath.montecarlo.conditionalexpectation.MonteCarloConditionalExpectationRegression;
import net.finmath.stochastic.ConditionalExpectationEstimator;
import net.finmath.stochastic.RandomVariable;

/**
 * Conditional expectation by least squares with the normal equations from ONE pass over the data ({@code fmhip_cross_moments},
 * DESIGN.md 4.8) instead of one product and one blocking average per pair of basis functions
 * ({@link MonteCarloConditionalExpectationRegression}: {@code b_i.mult(b_j).getAverage()}).
 *
 * The one-pass path is taken when every stochastic operand is a {@link RandomVariableHip}; deterministic basis functions are host
 * scalars folded through the constant-1 entry; beyond 12 basis functions the pass is {@code fmhip_cross_moments_wide} (DESIGN.md 4.14).
 * Foreign vectors, more than 60 basis functions, {@code FMHIP_DEVICE_WIDE_MOMENTS=0} beyond 12, or {@code FMHIP_DEVICE_CROSS_MOMENTS=0}
 * delegate to finmath-lib's own estimator.  The normal equations are solved on the host by the pivoted Cholesky the Python and C++
 * mirrors use (regression.py, host/regression.hpp): the largest remaining pivot next, and a basis function whose remaining pivot is
 * at most 1e-12 times the largest diagonal entry gets the coefficient 0.
 *
 * Not compiled in this repository (no JDK, no finmath-lib jar), like the rest of this directory.
 */
public class MonteCarloConditionalExpectationRegressionHip implements ConditionalExpectationEstimator {

	private static final int MAX_BASIS_FUNCTIONS = 12;          // fmhip_cross_moments
	private static final int MAX_BASIS_FUNCTIONS_WIDE = 60;     // fmhip_cross_moments_wide (DESIGN.md 4.14)
	private static final double PIVOT_TOLERANCE = 1e-12;

	private final RandomVariable[] basisFunctionsEstimator;
	private final RandomVariable[] basisFunctionsPredictor;

	public MonteCarloConditionalExpectationRegressionHip(final RandomVariable[] basisFunctions) {
		this(basisFunctions, basisFunctions);
	}

	public MonteCarloConditionalExpectationRegressionHip(final RandomVariable[] basisFunctionsEstimator, final RandomVariable[] basisFunctionsPredictor) {
		if(basisFunctionsEstimator.length != basisFunctionsPredictor.length) {
			throw new IllegalArgumentException("estimator and predictor need the same number of basis functions");
		}
		this.basisFunctionsEstimator = basisFunctionsEstimator.clone();
		this.basisFunctionsPredictor = basisFunctionsPredictor.clone();
	}

	static boolean deviceWideMoments() {
		return !"0".equals(System.getenv("FMHIP_DEVICE_WIDE_MOMENTS"));
	}

	static boolean deviceCrossMoments() {
		return !"0".equals(System.getenv("FMHIP_DEVICE_CROSS_MOMENTS"));
	}

	public RandomVariable getConditionalExpectation(final RandomVariable randomVariable) {
		final double[] beta = getLinearRegressionParameters(randomVariable);
		if(beta == null) {
			return new MonteCarloConditionalExpectationRegression(basisFunctionsEstimator, basisFunctionsPredictor).getConditionalExpectation(randomVariable);
		}
		RandomVariable conditionalExpectation = basisFunctionsPredictor[0].mult(beta[0]);
		for(int i = 1; i < basisFunctionsPredictor.length; i++) {
			conditionalExpectation = conditionalExpectation.addProduct(basisFunctionsPredictor[i], beta[i]);
		}
		return conditionalExpectation;
	}

	/** The coefficients from the one-pass normal equations, or null when the operands do not allow it (the caller delegates). */
	public double[] getLinearRegressionParameters(final RandomVariable dependent) {
		final int numberOfBasisFunctions = basisFunctionsEstimator.length;
		final boolean wide = numberOfBasisFunctions > MAX_BASIS_FUNCTIONS;
		if(!deviceCrossMoments() || numberOfBasisFunctions < 1 || numberOfBasisFunctions > MAX_BASIS_FUNCTIONS_WIDE || (wide && !deviceWideMoments())) return null;
		if(!(dependent instanceof RandomVariableHip) || dependent.isDeterministic()) return null;
		final long[] x = new long[numberOfBasisFunctions];
		final double[] scale = new double[numberOfBasisFunctions];
		RandomVariableHip sized = null;
		for(int i = 0; i < numberOfBasisFunctions; i++) {
			if(!(basisFunctionsEstimator[i] instanceof RandomVariableHip)) return null;
			final RandomVariableHip function = (RandomVariableHip) basisFunctionsEstimator[i];
			if(function.isDeterministic()) {
				x[i] = 0;
				scale[i] = function.doubleValue();
			}
			else {
				x[i] = function.deviceHandle();
				scale[i] = 1.0;
				sized = function;
			}
		}
		if(sized == null) return null;
		final double[] sums = new double[numberOfBasisFunctions * (numberOfBasisFunctions + 1) / 2 + numberOfBasisFunctions];
		final long[] y = new long[] { ((RandomVariableHip) dependent).deviceHandle() };
		Native.check(wide ? Native.crossMomentsWide(x, y, sums) : Native.crossMoments(x, y, sums));
		final double n = sized.expectationSampleSize();
		final double[][] a = new double[numberOfBasisFunctions][numberOfBasisFunctions];
		final double[] b = new double[numberOfBasisFunctions];
		int at = 0;
		for(int i = 0; i < numberOfBasisFunctions; i++) {
			for(int j = i; j < numberOfBasisFunctions; j++, at++) {
				a[i][j] = a[j][i] = sums[at] * (scale[i] * scale[j]) / n;
			}
		}
		for(int i = 0; i < numberOfBasisFunctions; i++) {
			b[i] = sums[at + i] * scale[i] / n;
		}
		return solveNormalEquations(a, b);
	}

	/** Cholesky with diagonal pivoting; regression.py: solve_normal_equations, step for step. */
	static double[] solveNormalEquations(final double[][] a, final double[] b) {
		final int size = b.length;
		final int[] perm = new int[size];
		final double[] d = new double[size];
		final double[][] l = new double[size][size];
		double largest = 0.0;
		for(int i = 0; i < size; i++) {
			perm[i] = i;
			d[i] = a[i][i];
			if(i == 0 || d[i] > largest) largest = d[i];
		}
		final double tolerance = PIVOT_TOLERANCE * largest;
		int rank = size;
		for(int k = 0; k < size; k++) {
			int p = k;
			for(int q = k + 1; q < size; q++) {
				if(d[perm[q]] > d[perm[p]]) p = q;
			}
			if(d[perm[p]] <= tolerance) {
				rank = k;
				break;
			}
			final int swap = perm[k]; perm[k] = perm[p]; perm[p] = swap;
			final int i = perm[k];
			l[i][k] = Math.sqrt(d[i]);
			for(int q = k + 1; q < size; q++) {
				final int j = perm[q];
				double s = a[j][i];
				for(int t = 0; t < k; t++) s -= l[j][t] * l[i][t];
				l[j][k] = s / l[i][k];
				d[j] -= l[j][k] * l[j][k];
			}
		}
		final double[] z = new double[rank];
		final double[] x = new double[size];
		for(int k = 0; k < rank; k++) {
			double s = b[perm[k]];
			for(int t = 0; t < k; t++) s -= l[perm[k]][t] * z[t];
			z[k] = s / l[perm[k]][k];
		}
		for(int k = rank - 1; k >= 0; k--) {
			double s = z[k];
			for(int t = k + 1; t < rank; t++) s -= l[perm[t]][k] * x[perm[t]];
			x[perm[k]] = s / l[perm[k]][k];
		}
		return x;
	}
}
