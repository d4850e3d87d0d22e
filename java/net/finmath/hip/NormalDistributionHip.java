package net.finmath.hip;

import java.util.function.DoubleUnaryOperator;

/**
 * The functions of the standard normal distribution that {@link RandomVariableHip#apply(DoubleUnaryOperator)} evaluates ON THE DEVICE —
 * the most common argument of {@code RandomVariable.apply} in finmath-lib is {@code NormalDistribution::cumulativeDistribution} — and the
 * closed-form option values built on them, per path: handed {@link #CUMULATIVE_DISTRIBUTION}, {@link #DENSITY} or
 * {@link #INVERSE_CUMULATIVE_DISTRIBUTION}, apply is one launch of {@code fmhip_function_apply} (DESIGN.md 4.21) and the vector never
 * leaves HBM; {@link #blackScholesGeneralizedOptionValue} and {@link #bachelierOptionValue} are one launch of
 * {@code fmhip_option_formula} on up to three vectors.
 *
 * The definition (host/normal_functions.hpp) is fp64 arithmetic written with + - * /, sqrt, an exp and a log that the host and the device
 * both compile; the device's bits are those of {@code Native.functionApplyHost} / {@code Native.optionFormulaHost}.  The formulas follow
 * finmath-lib's AnalyticFormulas, as remembered.
 *
 * UNCOMPILED / UNTESTED here: no JDK, no finmath-lib jar in the build image, like the rest of this directory.
 */
public final class NormalDistributionHip implements DoubleUnaryOperator {

	public static final int VALUE = 1, DELTA = 2, VEGA = 4;					// FMHIP_FORMULA_*
	public static final int BLACK_SCHOLES = 0, BACHELIER = 1;

	public static final NormalDistributionHip CUMULATIVE_DISTRIBUTION = new NormalDistributionHip(0);
	public static final NormalDistributionHip DENSITY = new NormalDistributionHip(1);
	public static final NormalDistributionHip INVERSE_CUMULATIVE_DISTRIBUTION = new NormalDistributionHip(2);

	private final int kind;													// FMHIP_FN_*

	private NormalDistributionHip(final int kind) { this.kind = kind; }

	int getKind() { return kind; }

	/** The definition at x, as the library's host entry point computes it for the fp32 number nearest to x. */
	@Override
	public double applyAsDouble(final double x) {
		final float[] out = new float[1];
		Native.check(Native.functionApplyHost(new float[] { (float)x }, new int[] { kind }, out));
		return out[0];
	}

	/** functions.length (1 ... 4) of the three at every path of x from ONE launch that reads x once: {CUMULATIVE_DISTRIBUTION, DENSITY} is value and derivative. */
	public static RandomVariableHip[] apply(final RandomVariableHip x, final NormalDistributionHip... functions) {
		final int[] kinds = new int[functions.length];
		for(int f = 0; f < functions.length; f++) kinds[f] = functions[f].kind;
		final long[] out = new long[functions.length];
		Native.check(Native.functionApply(x.deviceHandle(), kinds, out));
		final RandomVariableHip[] result = new RandomVariableHip[functions.length];
		for(int f = 0; f < functions.length; f++) result[f] = new RandomVariableHip(x.getFiltrationTime(), new DeviceVector(out[f], x.size()));
		return result;
	}

	/** payoffUnit (forward Phi(d+) - strike Phi(d-)) per path; forward, volatility and payoffUnit may be stochastic or constants, at least one stochastic. */
	public static RandomVariableHip blackScholesGeneralizedOptionValue(final RandomVariableHip forward, final RandomVariableHip volatility, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit) {
		return formula(BLACK_SCHOLES, forward, volatility, optionMaturity, optionStrike, payoffUnit, VALUE)[0];
	}

	/** payoffUnit ((forward - strike) Phi(d) + volatility sqrt(T) density(d)), d = (forward - strike) / (volatility sqrt(T)), per path. */
	public static RandomVariableHip bachelierOptionValue(final RandomVariableHip forward, final RandomVariableHip volatility, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit) {
		return formula(BACHELIER, forward, volatility, optionMaturity, optionStrike, payoffUnit, VALUE)[0];
	}

	/** One new vector per set bit of outputs (VALUE, DELTA, VEGA), in bit order, from ONE launch; the filtration time is the operands' maximum. */
	public static RandomVariableHip[] formula(final int model, final RandomVariableHip forward, final RandomVariableHip volatility, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit, final int outputs) {
		final RandomVariableHip[] operands = { forward, volatility, payoffUnit };
		final long[] handles = new long[3];
		final double[] scalars = new double[3];
		double time = Double.NEGATIVE_INFINITY;
		int size = 0;
		for(int k = 0; k < 3; k++) {
			time = Math.max(time, operands[k].getFiltrationTime());
			if(operands[k].isDeterministic()) scalars[k] = operands[k].doubleValue();
			else { handles[k] = operands[k].deviceHandle(); size = operands[k].size(); }
		}
		if(size == 0) throw new IllegalArgumentException("at least one of forward, volatility and payoffUnit is stochastic");
		final long[] out = new long[Integer.bitCount(outputs)];
		Native.check(Native.optionFormula(model, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], optionMaturity, optionStrike, outputs, out));
		final RandomVariableHip[] result = new RandomVariableHip[out.length];
		for(int f = 0; f < out.length; f++) result[f] = new RandomVariableHip(time, new DeviceVector(out[f], size));
		return result;
	}

	public static final int IMPLIED_VOLATILITY = 1, IMPLIED_D_PRICE = 2, IMPLIED_D_FORWARD = 4;			// FMHIP_IMPLIED_*

	/** The Black-Scholes volatility per path at which the call has optionValue (AnalyticFormulas.blackScholesOptionImpliedVolatility, as remembered); one launch of {@code fmhip_implied_volatility} (DESIGN.md 4.25). */
	public static RandomVariableHip blackScholesOptionImpliedVolatility(final RandomVariableHip forward, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit, final RandomVariableHip optionValue) {
		return impliedVolatility(BLACK_SCHOLES, optionValue, forward, optionMaturity, optionStrike, payoffUnit, IMPLIED_VOLATILITY)[0];
	}

	/** The Bachelier (normal) volatility per path at which the call has optionValue (AnalyticFormulas.bachelierOptionImpliedVolatility, as remembered). */
	public static RandomVariableHip bachelierOptionImpliedVolatility(final RandomVariableHip forward, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit, final RandomVariableHip optionValue) {
		return impliedVolatility(BACHELIER, optionValue, forward, optionMaturity, optionStrike, payoffUnit, IMPLIED_VOLATILITY)[0];
	}

	/** One new vector per set bit of outputs (IMPLIED_VOLATILITY, IMPLIED_D_PRICE, IMPLIED_D_FORWARD), in bit order, from ONE launch; the filtration time is the operands' maximum. */
	public static RandomVariableHip[] impliedVolatility(final int model, final RandomVariableHip optionValue, final RandomVariableHip forward, final double optionMaturity, final double optionStrike, final RandomVariableHip payoffUnit, final int outputs) {
		final RandomVariableHip[] operands = { optionValue, forward, payoffUnit };
		final long[] handles = new long[3];
		final double[] scalars = new double[3];
		double time = Double.NEGATIVE_INFINITY;
		int size = 0;
		for(int k = 0; k < 3; k++) {
			time = Math.max(time, operands[k].getFiltrationTime());
			if(operands[k].isDeterministic()) scalars[k] = operands[k].doubleValue();
			else { handles[k] = operands[k].deviceHandle(); size = operands[k].size(); }
		}
		if(size == 0) throw new IllegalArgumentException("at least one of optionValue, forward and payoffUnit is stochastic");
		final long[] out = new long[Integer.bitCount(outputs)];
		Native.check(Native.impliedVolatility(model, handles[0], scalars[0], handles[1], scalars[1], handles[2], scalars[2], optionMaturity, optionStrike, outputs, out));
		final RandomVariableHip[] result = new RandomVariableHip[out.length];
		for(int f = 0; f < out.length; f++) result[f] = new RandomVariableHip(time, new DeviceVector(out[f], size));
		return result;
	}
}
