package net.finmath.hip;

import net.finmath.stochastic.ConditionalExpectationEstimator;
import net.finmath.stochastic.RandomVariable;

/**
 * Conditional expectation by a least-squares fit PER BIN of a key random variable — the localized estimate finmath-lib's users reach
 * for where a global polynomial fails on a kinked continuation value (BermudanOption's binning basis, the
 * ...LocalizedOnDependentRegression factories).  The normal equations are block diagonal, one small block per bin; ONE pass over the
 * key and the data yields all of them ({@code fmhip_binned_cross_moments}, DESIGN.md 4.13), and ONE launch evaluates the piecewise
 * estimate as a new vector ({@code fmhip_binned_evaluate}) in the fp32 arithmetic of
 * {@code basis[0].mult(beta0).addProduct(basis[i], betai)}.
 *
 * Bins: {@code bounds.length + 1} of them, at most 64; a path with key k lies in bin #{ j : bounds[j] < k }.  Without bounds the bins hold
 * (nearly) equal counts: bounds[j-1] = sorted(key)[ceil(j*n/numberOfBins) - 1], taken by one {@code selectRanksBatch} call.  Every
 * operand is a {@link RandomVariableHip}, at most three basis functions; deterministic basis functions are host scalars folded through
 * the constant-1 entry.  Each block is solved by the pivoted Cholesky of {@link MonteCarloConditionalExpectationRegressionHip}, so an
 * empty bin gets coefficients 0.  The Python mirror (regression.py) also carries the generic path over any RandomVariable class.
 *
 * Not compiled in this repository (no JDK, no finmath-lib jar), like the rest of this directory.
 */
public class MonteCarloConditionalExpectationLocalizedRegressionHip implements ConditionalExpectationEstimator {

	private static final int MAX_BASIS_FUNCTIONS = 3;
	private static final int MAX_BINS = 64;

	private final RandomVariableHip key;
	private final double[] bounds;
	private final RandomVariable[] basisFunctionsEstimator;
	private final RandomVariable[] basisFunctionsPredictor;

	public MonteCarloConditionalExpectationLocalizedRegressionHip(final RandomVariable key, final int numberOfBins, final RandomVariable[] basisFunctions) {
		this(key, numberOfBins, basisFunctions, basisFunctions, null);
	}

	public MonteCarloConditionalExpectationLocalizedRegressionHip(final RandomVariable key, final int numberOfBins, final RandomVariable[] basisFunctionsEstimator,
			final RandomVariable[] basisFunctionsPredictor, final double[] bounds) {
		if(!(key instanceof RandomVariableHip) || key.isDeterministic()) throw new IllegalArgumentException("the key is a stochastic RandomVariableHip");
		if(numberOfBins < 1 || numberOfBins > MAX_BINS) throw new IllegalArgumentException("numberOfBins must be 1 ... " + MAX_BINS);
		if(basisFunctionsEstimator.length != basisFunctionsPredictor.length || basisFunctionsEstimator.length < 1 || basisFunctionsEstimator.length > MAX_BASIS_FUNCTIONS) {
			throw new IllegalArgumentException("estimator and predictor need the same number of basis functions, 1 ... " + MAX_BASIS_FUNCTIONS);
		}
		this.key = (RandomVariableHip) key;
		this.basisFunctionsEstimator = basisFunctionsEstimator.clone();
		this.basisFunctionsPredictor = basisFunctionsPredictor.clone();
		this.bounds = bounds != null ? bounds.clone() : quantileBounds(this.key, numberOfBins);
		if(this.bounds.length != numberOfBins - 1) throw new IllegalArgumentException("numberOfBins bins have numberOfBins - 1 bounds");
	}

	/** bounds[j-1] = sorted(key)[ceil(j*n/numberOfBins) - 1], j = 1 ... numberOfBins-1: one selection on the device. */
	public static double[] quantileBounds(final RandomVariableHip key, final int numberOfBins) {
		final double[] values = new double[numberOfBins - 1];
		if(numberOfBins == 1) return values;
		final long n = (long) key.expectationSampleSize();
		final long[] ranks = new long[numberOfBins - 1];
		for(int j = 1; j < numberOfBins; j++) ranks[j - 1] = Math.max((j * n + numberOfBins - 1) / numberOfBins - 1, 0);
		Native.check(Native.selectRanksBatch(new long[] { key.deviceHandle() }, ranks, values));
		return values;
	}

	private static long[] handles(final RandomVariable[] functions, final double[] scale) {
		final long[] x = new long[functions.length];
		for(int i = 0; i < functions.length; i++) {
			if(!(functions[i] instanceof RandomVariableHip)) throw new IllegalArgumentException("every basis function is a RandomVariableHip");
			final RandomVariableHip function = (RandomVariableHip) functions[i];
			x[i] = function.deviceHandle();
			if(scale != null) scale[i] = function.isDeterministic() ? function.doubleValue() : 1.0;
			else if(function.isDeterministic() && function.doubleValue() != 1.0) throw new IllegalArgumentException("a deterministic predictor is the constant 1");
		}
		return x;
	}

	/** beta[bin][i]: the coefficients of every bin's fit. */
	public double[][] getLinearRegressionParameters(final RandomVariable dependent) {
		if(!(dependent instanceof RandomVariableHip) || dependent.isDeterministic()) throw new IllegalArgumentException("the dependent is a stochastic RandomVariableHip");
		final int size = basisFunctionsEstimator.length, numberOfBins = bounds.length + 1, q = size * (size + 1) / 2 + size;
		final double[] scale = new double[size];
		final long[] x = handles(basisFunctionsEstimator, scale);
		final long[] counts = new long[numberOfBins];
		final double[] sums = new double[numberOfBins * q];
		Native.check(Native.binnedCrossMoments(key.deviceHandle(), bounds, x, new long[] { ((RandomVariableHip) dependent).deviceHandle() }, counts, sums));
		final double n = key.expectationSampleSize();
		final double[][] beta = new double[numberOfBins][];
		for(int bin = 0; bin < numberOfBins; bin++) {
			final double[][] a = new double[size][size];
			final double[] b = new double[size];
			int at = bin * q;
			for(int i = 0; i < size; i++) {
				for(int j = i; j < size; j++, at++) a[i][j] = a[j][i] = sums[at] * (scale[i] * scale[j]) / n;
			}
			for(int i = 0; i < size; i++) b[i] = sums[at + i] * scale[i] / n;
			beta[bin] = MonteCarloConditionalExpectationRegressionHip.solveNormalEquations(a, b);
		}
		return beta;
	}

	public RandomVariable getConditionalExpectation(final RandomVariable randomVariable) {
		final double[][] beta = getLinearRegressionParameters(randomVariable);
		final int size = basisFunctionsPredictor.length;
		final double[] coefficients = new double[beta.length * size];
		for(int bin = 0; bin < beta.length; bin++) System.arraycopy(beta[bin], 0, coefficients, bin * size, size);
		final long[] out = new long[1];
		Native.check(Native.binnedEvaluate(key.deviceHandle(), bounds, handles(basisFunctionsPredictor, null), coefficients, out));
		double time = key.getFiltrationTime();
		for(final RandomVariable function : basisFunctionsPredictor) time = Math.max(time, function.getFiltrationTime());
		return new RandomVariableHip(time, new DeviceVector(out[0], key.size()));
	}
}
