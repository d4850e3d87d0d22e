/*
 * UNCOMPILED SOURCE: no JDK and no finmath-lib jar were available where this was written; it has never been configured or compiled.
 * It states the binding the C++ and Python mirrors implement and test.
 */
package net.finmath.hip;

import net.finmath.montecarlo.BrownianMotion;
import net.finmath.stochastic.RandomVariable;
import net.finmath.time.TimeDiscretization;

/**
 * A Brownian motion whose increments come from a Sobol' sequence (Joe and Kuo's direction numbers, 1024 dimensions, digitally shifted by
 * the seed) through a Brownian bridge, or increment by increment, generated on the device (fmhip_bm_generate_sobol_device): what
 * finmath-lib's SobolSequence taken through BrownianMotionFromRandomNumberGenerator and BrownianBridge serve. Every increment equals the
 * host definition's (Native.sobolIncrementsHost) narrowed to float. numberOfTimeSteps * numberOfFactors is at most 1024.
 */
public class BrownianMotionFromSobolSequenceHip implements BrownianMotion {

	public static final int INCREMENTAL = 0, BRIDGE = 1;

	private final TimeDiscretization timeDiscretization;
	private final int numberOfFactors;
	private final int numberOfPaths;
	private final int seed;
	private final int construction;
	private final boolean randomize;
	private final long pathOffset;
	private transient RandomVariable[][] increments;
	private final Object lock = new Object();

	public BrownianMotionFromSobolSequenceHip(TimeDiscretization timeDiscretization, int numberOfFactors, int numberOfPaths, int seed, int construction, boolean randomize, long pathOffset) {
		this.timeDiscretization = timeDiscretization;
		this.numberOfFactors = numberOfFactors;
		this.numberOfPaths = numberOfPaths;
		this.seed = seed;
		this.construction = construction;
		this.randomize = randomize;
		this.pathOffset = pathOffset;
	}

	public BrownianMotionFromSobolSequenceHip(TimeDiscretization timeDiscretization, int numberOfFactors, int numberOfPaths, int seed) {
		this(timeDiscretization, numberOfFactors, numberOfPaths, seed, BRIDGE, true, 0L);
	}

	@Override
	public BrownianMotion getCloneWithModifiedSeed(int seed) {
		return new BrownianMotionFromSobolSequenceHip(timeDiscretization, numberOfFactors, numberOfPaths, seed, construction, randomize, pathOffset);
	}

	@Override
	public BrownianMotion getCloneWithModifiedTimeDiscretization(TimeDiscretization newTimeDiscretization) {
		return new BrownianMotionFromSobolSequenceHip(newTimeDiscretization, numberOfFactors, numberOfPaths, seed, construction, randomize, pathOffset);
	}

	@Override
	public RandomVariable getBrownianIncrement(int timeIndex, int factor) {
		synchronized (lock) {
			if (increments == null) generate();
		}
		return increments[timeIndex][factor];
	}

	private void generate() {
		final int steps = timeDiscretization.getNumberOfTimeSteps();
		final double[] dt = new double[steps];
		for (int i = 0; i < steps; i++) dt[i] = timeDiscretization.getTimeStep(i);
		final long[] handles = new long[steps * numberOfFactors];
		Native.check(Native.bmGenerateSobolDevice(seed, randomize ? 1 : 0, construction, steps, numberOfFactors, numberOfPaths, pathOffset, dt, handles));
		final RandomVariable[][] result = new RandomVariable[steps][numberOfFactors];
		for (int i = 0; i < steps; i++)
			for (int f = 0; f < numberOfFactors; f++)
				result[i][f] = new RandomVariableHip(timeDiscretization.getTime(i + 1), new DeviceVector(handles[i * numberOfFactors + f], numberOfPaths));
		increments = result;
	}

	@Override
	public RandomVariable getIncrement(int timeIndex, int factor) { return getBrownianIncrement(timeIndex, factor); }
	@Override
	public TimeDiscretization getTimeDiscretization() { return timeDiscretization; }
	@Override
	public int getNumberOfFactors() { return numberOfFactors; }
	@Override
	public int getNumberOfPaths() { return numberOfPaths; }
	@Override
	public RandomVariable getRandomVariableForConstant(double value) { return new RandomVariableHip(value); }
	public int getSeed() { return seed; }
	public int getConstruction() { return construction; }

	@Override
	public String toString() {
		return "BrownianMotionFromSobolSequenceHip [timeDiscretization=" + timeDiscretization + ", numberOfFactors=" + numberOfFactors + ", numberOfPaths=" + numberOfPaths
				+ ", seed=" + seed + ", construction=" + (construction == BRIDGE ? "bridge" : "incremental") + ", randomize=" + randomize + "]";
	}
}
