package net.finmath.hip;

import java.util.Arrays;
import java.util.function.DoubleUnaryOperator;

/**
 * A function tabulated on knots and interpolated — a local-volatility slice, a Markov-functional numeraire, a payoff profile, an exercise
 * boundary, an inverse empirical CDF — that {@link RandomVariableHip#apply(DoubleUnaryOperator)} evaluates ON THE DEVICE: handed an
 * instance of this class, apply is one launch of {@code fmhip_table_apply} (DESIGN.md 4.18) and the vector never leaves HBM; any other
 * operator is mapped on the host as before.
 *
 * The definition (host/tabulated_function.hpp): X = (double) x, s = the number of knots &lt;= X, t = X - knots[max(s - 1, 0)],
 * (float) (((C3 t + C2) t + C1) t + C0) with the four coefficients of segment s, every operation rounded on its own.  The coefficients come
 * from {@code fmhip_table_build}: interpolation PIECEWISE_CONSTANT, LINEAR, CUBIC_SPLINE (natural) or MONOTONE_CUBIC (Fritsch-Carlson),
 * extrapolation CONSTANT or LINEAR — names after finmath-lib's RationalFunctionInterpolation, as remembered.
 *
 * UNCOMPILED / UNTESTED here: no JDK, no finmath-lib jar in the build image, like the rest of this directory.
 */
public class TabulatedFunctionHip implements DoubleUnaryOperator {

	public enum InterpolationMethod { PIECEWISE_CONSTANT, LINEAR, CUBIC_SPLINE, MONOTONE_CUBIC }
	public enum ExtrapolationMethod { CONSTANT, LINEAR }

	private final double[] knots;
	private final double[] values;
	private final InterpolationMethod interpolationMethod;
	private final ExtrapolationMethod extrapolationMethod;
	private final int derivativeOrder;
	private final double[] coefficients;								// (knots.length + 1) segments of 4

	public TabulatedFunctionHip(final double[] knots, final double[] values) {
		this(knots, values, InterpolationMethod.LINEAR, ExtrapolationMethod.CONSTANT);
	}

	public TabulatedFunctionHip(final double[] knots, final double[] values, final InterpolationMethod interpolationMethod, final ExtrapolationMethod extrapolationMethod) {
		this(knots, values, interpolationMethod, extrapolationMethod, 0);
	}

	private TabulatedFunctionHip(final double[] knots, final double[] values, final InterpolationMethod interpolationMethod, final ExtrapolationMethod extrapolationMethod, final int derivativeOrder) {
		if(knots.length != values.length) throw new IllegalArgumentException(knots.length + " knots and " + values.length + " values");
		this.knots = knots.clone();
		this.values = values.clone();
		this.interpolationMethod = interpolationMethod;
		this.extrapolationMethod = extrapolationMethod;
		this.derivativeOrder = derivativeOrder;
		this.coefficients = new double[(knots.length + 1) * 4];
		Native.check(Native.tableBuild(this.knots, this.values, interpolationMethod.ordinal(), extrapolationMethod.ordinal(), derivativeOrder, coefficients));
	}

	/** The derivative of the interpolant on the same knots: the segments (C1, 2 C2, 3 C3, 0). */
	public TabulatedFunctionHip derivative() {
		if(derivativeOrder != 0) throw new UnsupportedOperationException("the derivative of a derivative is not tabulated");
		return new TabulatedFunctionHip(knots, values, interpolationMethod, extrapolationMethod, 1);
	}

	/** The definition's polynomial at the double x, not narrowed to fp32. */
	@Override
	public double applyAsDouble(final double x) {
		if(Double.isNaN(x)) return Double.NaN;
		int s = Arrays.binarySearch(knots, x);
		s = s >= 0 ? s + 1 : -s - 1;										// the number of knots <= x
		final double c0 = coefficients[4 * s], c1 = coefficients[4 * s + 1], c2 = coefficients[4 * s + 2], c3 = coefficients[4 * s + 3];
		if(c1 == 0.0 && c2 == 0.0 && c3 == 0.0) return c0;
		final double t = x - knots[Math.max(s - 1, 0)];
		return ((c3 * t + c2) * t + c1) * t + c0;
	}

	double[] getKnots() { return knots; }
	double[] getCoefficients() { return coefficients; }
}
