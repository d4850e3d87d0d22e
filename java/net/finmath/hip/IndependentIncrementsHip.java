/*
 * IndependentIncrementsHip.java — net.finmath.montecarlo.IndependentIncrements whose increments are generated ON the device, a law per
 * (time step, factor).  UNCOMPILED SOURCE, like the rest of java/: there is no JDK and no finmath-lib jar where it was written
 * (INTEGRATION.md); tests/test_jni_binding_cpu.py checks the native method it calls against the header.
 */
package net.finmath.hip;

import java.io.Serializable;
import java.util.function.IntFunction;

import net.finmath.montecarlo.IndependentIncrements;
import net.finmath.stochastic.RandomVariable;
import net.finmath.time.TimeDiscretization;

/**
 * Independent increments with a law per (time step, factor), generated on the device from finmath-lib's MT19937 stream
 * (fmhip_increments_generate_device) to the bits of the host definition (fmhip_increments_host): what
 * net.finmath.montecarlo.IndependentIncrementsFromICDF draws with one MersenneTwister.nextDouble() per increment, and on which
 * JumpProcessIncrements and the three-factor layout of MonteCarloMertonModel sit [unverified: restated from finmath-lib's documentation].
 *
 * The laws are the five the device knows: {@link Law#normal(double)}, {@link Law#uniform(double, double)}, {@link Law#poisson(double)},
 * {@link Law#gamma(double, double)}, {@link Law#exponential(double)} (an arbitrary inverse CDF, as finmath's class accepts, cannot be handed
 * to a kernel).  Poisson, uniform, gamma and exponential draws equal the host's — the gamma and exponential laws are defined in one header
 * the host and the device both compile (host/gamma_icdf.hpp) — normal draws are under the contract of
 * {@link BrownianMotionHip.Generator#MERSENNE_DEVICE}.  {@link #gammaProcess} and {@link #varianceGamma} lay out the factors of
 * finmath-lib's GammaProcess and VarianceGammaProcess [unverified: the variance-gamma factor layout is this project's].
 */
public class IndependentIncrementsHip implements IndependentIncrements, Serializable {

	private static final long serialVersionUID = 1L;

	/** A law of one increment: kind and two arguments, as fmhip.h states them. */
	public static final class Law implements Serializable {
		private static final long serialVersionUID = 1L;
		public static final int NORMAL = 0, UNIFORM = 1, POISSON = 2, GAMMA = 4, EXPONENTIAL = 5;      // 3 is no law
		final int kind;
		final double a, b;
		private Law(final int kind, final double a, final double b) { this.kind = kind; this.a = a; this.b = b; }
		/** inverse normal CDF times scale: sqrt(dt) for a Brownian factor, 1 for a jump size */
		public static Law normal(final double scale) { return new Law(NORMAL, scale, 0.0); }
		public static Law uniform(final double lowerBound, final double upperBound) { return new Law(UNIFORM, lowerBound, upperBound); }
		/** a jump count with the given mean (lambda * dt), at most 128 */
		public static Law poisson(final double mean) { return new Law(POISSON, mean, 0.0); }
		/** inverse regularised incomplete gamma function times scale; 0.01 <= shape <= 1000, scale finite and positive */
		public static Law gamma(final double shape, final double scale) { return new Law(GAMMA, shape, scale); }
		/** -log(1 - u) / rate; rate finite and positive */
		public static Law exponential(final double rate) { return new Law(EXPONENTIAL, rate, 0.0); }
	}

	private final TimeDiscretization timeDiscretization;
	private final int numberOfFactors;
	private final int numberOfPaths;
	private final int seed;
	private final long pathOffset;
	private final IntFunction<IntFunction<Law>> laws;

	private transient RandomVariable[][] increments;
	private final Object incrementsLazyInitLock = new Object();

	/**
	 * @param laws timeIndex -> factor -> law of that increment
	 * @param pathOffset this object holds paths pathOffset ... pathOffset + numberOfPaths of the whole process (a rank's block)
	 */
	public IndependentIncrementsHip(final TimeDiscretization timeDiscretization, final int numberOfFactors, final int numberOfPaths, final int seed,
			final IntFunction<IntFunction<Law>> laws, final long pathOffset) {
		this.timeDiscretization = timeDiscretization;
		this.numberOfFactors = numberOfFactors;
		this.numberOfPaths = numberOfPaths;
		this.seed = seed;
		this.laws = laws;
		this.pathOffset = pathOffset;
	}

	public IndependentIncrementsHip(final TimeDiscretization timeDiscretization, final int numberOfFactors, final int numberOfPaths, final int seed,
			final IntFunction<IntFunction<Law>> laws) {
		this(timeDiscretization, numberOfFactors, numberOfPaths, seed, laws, 0L);
	}

	/** The three factors of a Merton jump-diffusion: Brownian increment, standard normal jump size, Poisson jump count with mean lambda * dt. */
	public static IndependentIncrementsHip merton(final TimeDiscretization timeDiscretization, final int numberOfPaths, final int seed, final double jumpIntensity) {
		return new IndependentIncrementsHip(timeDiscretization, 3, numberOfPaths, seed, timeIndex -> factor ->
			factor == 0 ? Law.normal(Math.sqrt(timeDiscretization.getTimeStep(timeIndex))) : factor == 1 ? Law.normal(1.0) : Law.poisson(jumpIntensity * timeDiscretization.getTimeStep(timeIndex)));
	}

	/** One factor: a gamma process, increment i ~ Gamma(shapePerTime * dt_i, scale). */
	public static IndependentIncrementsHip gammaProcess(final TimeDiscretization timeDiscretization, final int numberOfPaths, final int seed, final double shapePerTime, final double scale) {
		return new IndependentIncrementsHip(timeDiscretization, 1, numberOfPaths, seed, timeIndex -> factor ->
			Law.gamma(shapePerTime * timeDiscretization.getTimeStep(timeIndex), scale));
	}

	/** The two factors of a variance-gamma process: factor 0 the gamma clock Gamma(dt_i / nu, nu), factor 1 a standard normal. */
	public static IndependentIncrementsHip varianceGamma(final TimeDiscretization timeDiscretization, final int numberOfPaths, final int seed, final double nu) {
		return new IndependentIncrementsHip(timeDiscretization, 2, numberOfPaths, seed, timeIndex -> factor ->
			factor == 0 ? Law.gamma(timeDiscretization.getTimeStep(timeIndex) / nu, nu) : Law.normal(1.0));
	}

	/** theta * Gamma_i + sigma * sqrt(Gamma_i) * Z_i from increments laid out by {@link #varianceGamma}, in RandomVariable methods. */
	public static RandomVariable varianceGammaIncrement(final IndependentIncrements increments, final int timeIndex, final double sigma, final double theta) {
		final RandomVariable gamma = increments.getIncrement(timeIndex, 0);
		return gamma.mult(theta).addProduct(gamma.sqrt().mult(increments.getIncrement(timeIndex, 1)), sigma);
	}

	@Override
	public RandomVariable getIncrement(final int timeIndex, final int factor) {
		synchronized(incrementsLazyInitLock) {
			if(increments == null) {
				doGenerateIncrements();
			}
		}
		return increments[timeIndex][factor];
	}

	private void doGenerateIncrements() {
		final int numberOfTimeSteps = timeDiscretization.getNumberOfTimeSteps();
		final int[] kinds = new int[numberOfTimeSteps * numberOfFactors];
		final double[] a = new double[kinds.length];
		final double[] b = new double[kinds.length];
		for(int timeIndex = 0; timeIndex < numberOfTimeSteps; timeIndex++) {
			for(int factor = 0; factor < numberOfFactors; factor++) {
				final Law law = laws.apply(timeIndex).apply(factor);
				kinds[timeIndex * numberOfFactors + factor] = law.kind;
				a[timeIndex * numberOfFactors + factor] = law.a;
				b[timeIndex * numberOfFactors + factor] = law.b;
			}
		}
		final long[] handles = new long[kinds.length];
		Native.check(Native.incrementsGenerateDevice(seed, numberOfTimeSteps, numberOfFactors, numberOfPaths, pathOffset, kinds, a, b, handles));
		final RandomVariable[][] generated = new RandomVariable[numberOfTimeSteps][numberOfFactors];
		for(int timeIndex = 0; timeIndex < numberOfTimeSteps; timeIndex++) {
			final double time = timeDiscretization.getTime(timeIndex + 1);
			for(int factor = 0; factor < numberOfFactors; factor++) {
				generated[timeIndex][factor] = new RandomVariableHip(time, new DeviceVector(handles[timeIndex * numberOfFactors + factor], numberOfPaths));
			}
		}
		increments = generated;
	}

	@Override
	public TimeDiscretization getTimeDiscretization() { return timeDiscretization; }

	@Override
	public int getNumberOfFactors() { return numberOfFactors; }

	@Override
	public int getNumberOfPaths() { return numberOfPaths; }

	@Override
	public RandomVariable getRandomVariableForConstant(final double value) { return new RandomVariableHip(value); }

	@Override
	public IndependentIncrements getCloneWithModifiedSeed(final int seed) {
		return new IndependentIncrementsHip(timeDiscretization, numberOfFactors, numberOfPaths, seed, laws, pathOffset);
	}

	@Override
	public IndependentIncrements getCloneWithModifiedTimeDiscretization(final TimeDiscretization newTimeDiscretization) {
		return new IndependentIncrementsHip(newTimeDiscretization, numberOfFactors, numberOfPaths, seed, laws, pathOffset);
	}

	public int getSeed() { return seed; }

	public long getPathOffset() { return pathOffset; }
}
