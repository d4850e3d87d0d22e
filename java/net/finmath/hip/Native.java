/*
 * Native.java — 1:1 image of include/fmhip.h (the C-ABI of libfmhip.so): one static native method per exported function,
 * no logic.  The JNI side is src/jni/fmhip_jni.cpp (one Java_net_finmath_hip_Native_* function per method).
 *
 * UNCOMPILED / UNTESTED in this repository: the build image has no JDK, no jni.h and no finmath-lib jar (DESIGN.md §1).
 * What IS checked here, on every test run: that this class, the JNI file and the header declare exactly the same set of
 * entry points (tests/test_jni_binding_cpu.py).
 *
 * Naming: fmhip_vec_create_from_double → vecCreateFromDouble.  Conventions:
 *   - functions that CREATE a vector or a program return the new handle (0 = failure, see lastError()): they are the hot path
 *     of every RandomVariable method and must not allocate an out-array per call;
 *   - every other function returns the C status (0 = FMHIP_OK) and writes results into caller-provided arrays;
 *   - device pointers and streams travel as long.
 * Replaces the JCuda / JCurand imports of RandomVariableCuda.java:8-16 and BrownianMotionCudaWithRandomVariableCuda.java:153-181.
 */
package net.finmath.hip;

final class Native {

	static {
		System.loadLibrary("fmhip_jni");		// libfmhip_jni.so, linked against libfmhip.so
	}

	private Native() { }

	// ---- lifecycle (fmhip.h: fmhip_init … fmhip_get_stream)
	static native int init(int deviceIndex);
	static native int initDevices(int[] devices);
	static native int deviceCount(int[] count);
	static native int    setThreadEngines(int enabled, int[] previous);   // fmhip_set_thread_engines: an engine per caller thread
	static native int shutdown();
	static native int isInitialized();
	static native int abiVersion();
	static native String lastError();
	static native int deviceInfo(String[] name, int[] computeUnits, long[] hbmBytes);
	static native int synchronize();
	static native int getStream(long[] stream);

	// ---- vectors
	static native long vecCreateFromDouble(double[] values);
	static native long vecCreateFromFloat(float[] values);
	static native long vecCreateFilled(long n, double value);
	static native long vecCreateUninitialized(long n);
	static native int vecRetain(long vector);
	static native int vecRelease(long vector);
	static native int vecSize(long vector, long[] size);
	static native int vecReadDouble(long vector, double[] out);
	static native int vecReadFloat(long vector, float[] out);
	static native int vecDevicePtr(long vector, long[] devicePointer);

	// ---- element-wise operations (replace callFunctionv1s0 … v2s1, RandomVariableCuda.java:483-557)
	static native long callV1s0(int opcode, long a);
	static native long callV1s1(int opcode, long a, double s);
	static native long callV2s0(int opcode, long a, long b);
	static native long callV2s1(int opcode, long a, long b, double s);
	static native long callV3s0(int opcode, long a, long b, long c);

	// ---- lazy fusion front-end
	static native int setFusion(int enabled, int[] previous);
	static native int flush();
	static native int fusionHold(int hold, int[] previous);
	static native int setStepGrouping(int steps, int[] previous);
	static native int graphClone(long[] roots, int nCopies, long[] leafFrom, long[] leafTo, double[] scalarsOrNull, int nScalars, long[] out);
	static native int graphScalars(long[] roots, double[] scalarsOutOrNull, int[] count);
	static native int setMathMode(int mode, int[] previous);

	// ---- reductions: {sum, sumsq, min, max} per vector (replace getAverage … getMax, RandomVariableCuda.java:830-901)
	static native int reduceMoments(long vector, double shift, double[] moments4);
	static native int reduceMomentsDevice(long vector, double shift, long deviceOut4Doubles);
	static native int reduceMomentsBatch(long[] vectors, double[] shiftsOrNull, double[] moments4PerVector);
	static native int reduceMomentsBatchDevice(long[] vectors, double[] shiftsOrNull, long deviceOut);
	// ---- order statistics on the device (replace the download-and-sort of getQuantile / getQuantileExpectation / getHistogram, RandomVariableCuda.java:970-1091)
	/** valuesOut[k * ranks.length + j] = the element at 0-based position ranks[j] of the ascending sample of vectors[k] (Arrays.sort order). */
	static native int selectRanksBatch(long[] vectors, long[] ranks, double[] valuesOut);
	/** sumsOut[k] = the fp64 sum of the positions rankFrom..rankTo (inclusive) of the ascending sample of vectors[k]. */
	static native int rankSumsBatch(long[] vectors, long rankFrom, long rankTo, double[] sumsOut);
	/** countsOut[j] = number of elements x with (double) x <= bounds[j]; NaN elements are not counted. */
	static native int countNotAbove(long vector, double[] bounds, long[] countsOut);
	// ---- cross moments: the normal equations of a regression in one pass (replace b_i.mult(b_j).getAverage() per pair, MonteCarloConditionalExpectationRegression)
	/** sumsOut = the x.length(x.length+1)/2 sums of x_i*x_j (i <= j, row-major) followed by the x.length*y.length sums of x_i*y_m; a handle of 0 in x is the constant 1. */
	static native int crossMoments(long[] x, long[] y, double[] sumsOut);
	/** crossMoments for x.length + y.length <= 64 (fmhip_cross_moments_wide: one pass on the matrix cores); same layout, its own bits. */
	static native int crossMomentsWide(long[] x, long[] y, double[] sumsOut);
	// ---- localized regression: the cross moments per bin of a key vector in one pass, and the piecewise estimate as a new vector (MonteCarloConditionalExpectationLocalizedRegressionHip)
	/** bin(k) = number of bounds below k (bounds.length + 1 bins, at most 64; bounds may be null for one bin).  countsOut[b] = paths in bin b; sumsOut[b*q ...] = the sums of crossMoments over the paths of bin b, q = x.length(x.length+1)/2 + x.length*y.length; x.length <= 3, y.length <= 4. */
	static native int binnedCrossMoments(long key, double[] bounds, long[] x, long[] y, long[] countsOut, double[] sumsOut);
	/** The definition of binnedCrossMoments over host arrays: xColumns (yColumns) holds nX (nY) columns of key.length floats; bit i of onesMask makes x_i the constant 1. */
	static native int binnedCrossMomentsHost(float[] key, double[] bounds, float[] xColumns, int nX, int onesMask, float[] yColumns, int nY, long[] countsOut, double[] sumsOut);
	/** out[0] = a new vector: ((x_0*c_0) + x_1*c_1) + x_2*c_2 per path with c = (float) coefficients[bin(key)*x.length + i], every fp32 operation rounded on its own. */
	static native int binnedEvaluate(long key, double[] bounds, long[] x, double[] coefficients, long[] out);
	/** The definition of binnedEvaluate over host arrays (columns as in binnedCrossMomentsHost). */
	static native int binnedEvaluateHost(float[] key, double[] bounds, float[] xColumns, int nX, int onesMask, double[] coefficients, float[] out);
	// ---- sort on the device: a stable radix sort of (key, path index) pairs by the key of the order statistics; ties keep path order, NaNs last
	/** sortedKeyOut[0] (may be null when values.length > 0) and sortedValuesOut[i] = new vectors out[r] = in[permutation[r]], copied bit for bit; values.length <= 8. */
	static native int sortByKey(long key, long[] values, long[] sortedKeyOut, long[] sortedValuesOut);
	/** permutationOut[r] = the path at position r of the ascending sample; permutationOut.length = the vector's size. */
	static native int argsort(long key, long[] permutationOut);
	/** The definition of argsort over a host array. */
	static native int argsortHost(float[] key, long[] permutationOut);
	/** out[0] = a new vector: (float) ((rank(p) + 0.5) / n) per path, ordinal ranks (ties by path index). */
	static native int rankScores(long key, long[] out);
	/** out[j] = (double) v[positions[j]]; every position in [0, size). */
	static native int vecReadElements(long v, long[] positions, double[] out);
	// ---- prefix sums on the device: P[r] = the fp64 sum of v[0..r] in a tree that is a function of the size alone; non-decreasing for input without negative elements
	/** out[0] = a new vector: (float) P[r], or with mode 1 (float) (P[r] / (r + 1)); totalOutOrNull[0] = P[size - 1]. */
	static native int prefixSums(long v, int mode, long[] out, double[] totalOutOrNull);
	/** sumsOut[j] = P[positions[j]]; 1 ... 4096 positions in [0, size). */
	static native int prefixSumsAt(long v, long[] positions, double[] sumsOut);
	/** positionsOut[j] = the smallest r with P[r] >= thresholds[j] (times P[size - 1] when relative), sumsOut[j] = that P[r]; size and P[size - 1] if there is none. */
	static native int prefixSearch(long v, double[] thresholds, boolean relative, long[] positionsOut, double[] sumsOut, double[] totalOutOrNull);
	/** The definition of the prefix sums over a host array. */
	static native int prefixSumsHost(float[] v, double[] prefixOut);
	// ---- resampling on the device: ancestors drawn from the cumulative weights (systematic, stratified, multinomial; equal weights: the bootstrap), state vectors gathered along
	/** valuesOut[i] = a new vector of m elements, values[i][a_j] bit for bit (values.length <= 8); ancestorsOutOrNull[0] = the ancestors as floats (n <= 2^24); totalOutOrNull[0] = the total weight (not positive or infinite: every output is NaN).  weights == 0: equal weights; scheme 0 systematic (offset in [0, 1), uniforms not read), 1 stratified, 2 multinomial (uniforms: m elements).  The bits are those of resampleHost. */
	static native int resample(long weights, int scheme, long m, double offset, long uniforms, long[] values, long[] valuesOut, long[] ancestorsOutOrNull, double[] totalOutOrNull);
	/** The definition of resample over host arrays: valueColumns holds nValues columns of n floats, outColumns nValues columns of m floats; ancestorsOutOrNull[j] = a_j, -1 for a dead element. */
	static native int resampleHost(float[] weightsOrNull, long n, int scheme, long m, double offset, float[] uniformsOrNull, float[] valueColumns, int nValues, float[] outColumns, long[] ancestorsOutOrNull, double[] totalOutOrNull);
	// ---- selection on the device: the paths on which mask >= 0 as shorter vectors (copy_if), back again, and a gather by an index; the device's bits are those of the Host twins
	/** valuesOutOrNull[i] = a new vector of count elements, the selected paths of values[i] in path order, bit for bit (at most 8 vectors; none: null); positionsOutOrNull[0] = their positions as floats (n <= 2^24); countOutOrNull[0] = count.  count == 0: every handle is 0, nothing is allocated. */
	static native int compress(long mask, long[] valuesOrNull, long[] valuesOutOrNull, long[] positionsOutOrNull, long[] countOutOrNull);
	/** The inverse of compress: valuesOut[i] = a new vector of the mask's size, values[i][q(r)] on the selected paths and (float) fill elsewhere; values of another size than the mask's count: FMHIP_ERR_SIZE_MISMATCH. */
	static native int expand(long mask, long[] values, double fill, long[] valuesOut);
	/** valuesOut[i][j] = values[i][index[j]] bit for bit where index[j] is an integer in [0, n - 1], the quiet NaN elsewhere; the status does not depend on the index. */
	static native int gather(long index, long[] values, long[] valuesOut);
	/** The definition of compress over host arrays: valueColumns and outColumns hold nValues columns of mask.length floats; the first countOutOrNull[0] elements of each output column and of positionsOutOrNull are written. */
	static native int compressHost(float[] mask, float[] valueColumns, int nValues, float[] outColumns, long[] positionsOutOrNull, long[] countOutOrNull);
	/** The definition of expand over host arrays: valueColumns holds nValues columns of nValueElements floats, outColumns nValues columns of mask.length floats. */
	static native int expandHost(float[] mask, float[] valueColumns, int nValues, long nValueElements, double fill, float[] outColumns);
	/** The definition of gather over host arrays: valueColumns holds nValues columns of n floats, outColumns nValues columns of index.length floats. */
	static native int gatherHost(float[] index, float[] valueColumns, int nValues, long n, float[] outColumns);
	// ---- reduce by key on the device: count, sum, mean and variance per group of an index vector; the device's bits are those of the Host twin
	/** Per group k of m (index[j] == k; anything that is no integer in [0, m - 1] belongs to no group): countsOutOrNull[0] = a new vector of m counts, outs[i * popcount(mask) + j] = a new vector of m elements, output j (the set bits of mask ascending: 1 sum, 2 mean, 4 variance) of values[i] (at most 4 vectors; none: null); ungroupedOutOrNull[0] = the elements of no group. */
	static native int groupSums(long index, long m, long[] valuesOrNull, int mask, long[] countsOutOrNull, long[] outsOrNull, long[] ungroupedOutOrNull);
	/** The definition of groupSums over host arrays: valueColumns holds nValues columns of index.length floats, outColumns nValues * popcount(mask) columns of m floats, countsOutOrNull m floats. */
	static native int groupSumsHost(float[] index, long m, float[] valueColumns, int nValues, int mask, float[] countsOutOrNull, float[] outColumns, long[] ungroupedOutOrNull);
	// ---- tabulated functions on the device: RandomVariable.apply for a curve; the device's bits are those of tableApplyHost
	/** coefficientsOut[(knots.length + 1) * 4]: the segments of one function from its values at the knots; interpolation 0 piecewise constant, 1 linear, 2 natural cubic spline, 3 monotone cubic; extrapolation 0 constant, 1 linear; derivative 0 or 1. */
	static native int tableBuild(double[] knots, double[] values, int interpolation, int extrapolation, int derivative, double[] coefficientsOut);
	/** out[f] = a new vector: function f of coefficients[nTables][knots.length + 1][4] at every element of x; 1 ... 4 functions on the same knots from one launch that reads x once. */
	static native int tableApply(long x, double[] knots, double[] coefficients, int nTables, long[] out);
	/** The definition of tableApply over a host array: outColumns holds nTables columns of x.length floats. */
	static native int tableApplyHost(float[] x, double[] knots, double[] coefficients, int nTables, float[] outColumns);
	// ---- named functions and option formulas per path: the normal distribution function, density and quantile; Black-Scholes and Bachelier
	/** out[f] = a new vector: function kinds[f] (0 normal distribution function, 1 its density, 2 its quantile) at every element of x; 1 ... 4 functions from one launch that reads x once. */
	static native int functionApply(long x, int[] kinds, long[] out);
	/** The definition of functionApply over a host array: outColumns holds kinds.length columns of x.length floats. */
	static native int functionApplyHost(float[] x, int[] kinds, float[] outColumns);
	/** out = one new vector per set bit of outputs (1 value, 2 delta, 4 vega), in bit order: the call of model 0 (Black-Scholes) or 1 (Bachelier) in forward form; an operand handle of 0 is the scalar beside it, at least one is a vector. */
	static native int optionFormula(int model, long forward, double forwardScalar, long volatility, double volatilityScalar, long payoffUnit, double payoffUnitScalar, double maturity, double strike, int outputs, long[] out);
	/** The definition of optionFormula over host arrays of n floats; an operand array that is null is the scalar beside it; outColumns holds one column of n floats per set bit. */
	static native int optionFormulaHost(int model, float[] forwardOrNull, double forwardScalar, float[] volatilityOrNull, double volatilityScalar, float[] payoffUnitOrNull, double payoffUnitScalar, int n, double maturity, double strike, int outputs, float[] outColumns);
	// ---- implied volatility per path: the inverse of optionFormula's value in the volatility
	/** out = one new vector per set bit of outputs (1 volatility, 2 its partial in the price, 4 its partial in the forward), in bit order: the volatility at which the call of model 0 (Black-Scholes) or 1 (Bachelier) has the given price; an operand handle of 0 is the scalar beside it, at least one is a vector. */
	static native int impliedVolatility(int model, long price, double priceScalar, long forward, double forwardScalar, long payoffUnit, double payoffUnitScalar, double maturity, double strike, int outputs, long[] out);
	/** The definition of impliedVolatility over host arrays of n floats; an operand array that is null is the scalar beside it; outColumns holds one column of n floats per set bit. */
	static native int impliedVolatilityHost(int model, float[] priceOrNull, double priceScalar, float[] forwardOrNull, double forwardScalar, float[] payoffUnitOrNull, double payoffUnitScalar, int n, double maturity, double strike, int outputs, float[] outColumns);
	// ---- transform option value per path: a call under a model with an exponential-affine transform (Black-Scholes, Merton, Heston, Bates, double Heston) as a finite sum over a node table
	/** out = one new vector per set bit of outputs (1 value, 2 its partial in the forward, 4 its partial in the first state), in bit order; nodes holds nNodes rows of 3 + 2 nStates doubles (u, a_re, a_im, b_re[], b_im[]); states and stateScalars hold nStates entries (null for none); an operand handle of 0 is the scalar beside it, at least one is a vector. */
	static native int transformOption(double[] nodes, int nNodes, int nStates, long forward, double forwardScalar, long[] statesOrNull, double[] stateScalarsOrNull, long payoffUnit, double payoffUnitScalar, double strike, int outputs, long[] out);
	/** The definition of transformOption over host arrays of n floats; an operand array that is null is the scalar beside it; outColumns holds one column of n floats per set bit. */
	static native int transformOptionHost(double[] nodes, int nNodes, int nStates, float[] forwardOrNull, double forwardScalar, float[] state0OrNull, float[] state1OrNull, double[] stateScalarsOrNull, float[] payoffUnitOrNull, double payoffUnitScalar, int n, double strike, int outputs, float[] outColumns);
	// ---- nested simulation: the moments of consecutive blocks as new vectors, and the repeat that starts k inner paths per outer state
	/** outs[i * popcount(mask) + j] = a new vector of n / block elements: output j (mask bits in ascending order: 1 sum, 2 mean, 4 population variance) of the consecutive blocks of vs[i]; 1 ... 4 vectors of one size, each read once; the bits are those of blockMomentsHost. */
	static native int blockMoments(long[] vs, long block, int mask, long[] outs);
	/** The definition of blockMoments over a host array: outColumns holds one column of v.length / block floats per set bit of mask. */
	static native int blockMomentsHost(float[] v, long block, int mask, float[] outColumns);
	/** out[0] = a new vector of n * each * times elements: out[(t * n + p) * each + e] = v[p], copied bit for bit. */
	static native int vecRepeat(long v, long each, long times, long[] out);
	// ---- block order statistics: ranks and range means of consecutive blocks (at most 4096 elements) as new vectors, and the blocks sorted
	/** outs[i * (ranks.length + rangeFrom.length) + j] = a new vector of n / block elements, ranks first: the element at rank ranks[j] of every ascending-sorted block of vs[i] (the order of Arrays.sort(float[])), resp. the mean of its ranks rangeFrom[j] ... rangeTo[j]; 1 ... 4 vectors of one size, 0 ... 8 ranks, 0 ... 4 ranges, at least one; the bits are those of blockOrderStatisticsHost. */
	static native int blockOrderStatistics(long[] vs, long block, long[] ranks, long[] rangeFrom, long[] rangeTo, long[] outs);
	/** The definition of blockOrderStatistics over a host array: outColumns holds one column of v.length / block floats per rank, then per range. */
	static native int blockOrderStatisticsHost(float[] v, long block, long[] ranks, long[] rangeFrom, long[] rangeTo, float[] outColumns);
	/** out[0] = a new vector of n elements: every block of `block` elements of v sorted ascending; every NaN comes back as the quiet NaN. */
	static native int blockSort(long v, long block, long[] out);
	/** The definition of blockSort over a host array. */
	static native int blockSortHost(float[] v, long block, float[] out);
	// ---- order statistics across vectors: the ranks of the K values of every path as values and as slots, and the element an index names
	/** outs = new vectors of n elements: for every selector ranks[j] (0 ... K - 1, duplicates allowed) the ranks[j]-th smallest of vs[0][p] ... vs[K-1][p] (the order of Arrays.sort(float[]), ties by slot) if outputs has bit 1, then the slot it came from as a float if outputs has bit 2; K = vs.length = 1 ... 32, 1 ... 32 selectors; the bits are those of crossOrderStatisticsHost. */
	static native int crossOrderStatistics(long[] vs, int[] ranks, int outputs, long[] outs);
	/** The definition of crossOrderStatistics over host arrays: vsColumns holds nVs columns of n floats, outColumns one column of n floats per output. */
	static native int crossOrderStatisticsHost(float[] vsColumns, int nVs, int[] ranks, int outputs, float[] outColumns);
	/** out[0] = a new vector: out[p] = vs[j][p] bit for bit where index[p] is an integer j in [0, vs.length), the quiet NaN for every other index[p]. */
	static native int crossSelect(long index, long[] vs, long[] out);
	/** The definition of crossSelect over host arrays: vsColumns holds nVs columns of index.length floats. */
	static native int crossSelectHost(float[] index, float[] vsColumns, int nVs, float[] out);
	// ---- kernel regression: kernel-weighted local moments of up to 4 vectors at up to 256 points of a key from one launch
	/** sumsOut[points.length][order 0: 1 + y.length; order 1: 3 + 2 y.length]: per point the fp64 sums [w, w*y...] or [w, w*d, w*d*d, w*y..., w*d*y...] over its members (lower &lt; key &lt; upper); kernel 0 uniform, 1 triangular, 2 Epanechnikov, 3 quartic, 4 triweight. */
	static native int kernelMoments(long key, double[] points, double[] bandwidths, int kernel, int order, long[] y, double[] sumsOut);
	/** The definition of kernelMoments over host arrays: yColumns holds nY columns of key.length floats. */
	static native int kernelMomentsHost(float[] key, double[] points, double[] bandwidths, int kernel, int order, float[] yColumns, int nY, double[] sumsOut);
	// ---- polynomial regression in one pass: the normal equations of a polynomial basis from the state vectors, the monomials formed in registers
	/** crossMomentsWide for the regressors [monomials of states..., extraX...] and the dependents y; exponents holds states.length ints (0 ... 6) per monomial, a row of zeros is the constant 1; a handle of 0 in extraX is the constant 1.  Bit for bit the sums of crossMomentsWide on the materialised monomials. */
	static native int polynomialCrossMoments(long[] states, int[] exponents, long[] extraX, long[] y, double[] sumsOut);
	/** out[0] = a new vector: ((t_0*c_0) + t_1*c_1) + ... over the monomials, then extraX, c = (float) coefficients[i], every fp32 operation rounded on its own. */
	static native int polynomialEvaluate(long[] states, int[] exponents, long[] extraX, double[] coefficients, long[] out);
	/** The definition of polynomialCrossMoments over host arrays: stateColumns (extraColumns, yColumns) holds nStates (nExtra, nY) columns of equal length; bit i of onesMask makes extra i the constant 1. */
	static native int polynomialCrossMomentsHost(float[] stateColumns, int nStates, int[] exponents, float[] extraColumns, int nExtra, int onesMask, float[] yColumns, int nY, double[] sumsOut);
	/** The definition of polynomialEvaluate over host arrays (columns as in polynomialCrossMomentsHost). */
	static native int polynomialEvaluateHost(float[] stateColumns, int nStates, int[] exponents, float[] extraColumns, int nExtra, int onesMask, double[] coefficients, float[] out);
	/** With a device list: one device buffer per listed device (0 = not wanted there), each receives the moments of the whole vectors. */
	static native int reduceMomentsBatchDevices(long[] vectors, double[] shiftsOrNull, long[] deviceOutPerDevice);
	static native int getStreamOf(int shard, long[] stream);
	/** kind[0]: 0 = one device, 1 = grouped RCCL all-gather over the listed devices, 2 = combined on the host. */
	static native int expectationCollective(int[] kind);
	// the same reduction in two halves: begin enqueues and returns a ticket (ticket[0]); end waits for that reduction only and retires the ticket
	static native int reduceMomentsBatchBegin(long[] vectors, double[] shiftsOrNull, long[] ticket);
	static native int vecGiveUpValues(long[] vectors);
	static native int reduceMomentsBatchEnd(long ticket, double[] moments4PerVector, int count);
	// expectation communicator (paths sharded over processes): gatherFunction = address of a C function of type fmhip_gather_fn,
	// e.g. from an MPI / RCCL helper library; context is handed back to it.  0 removes the communicator.
	static native int setExpectationComm(int world, int rank, long gatherFunction, long context);
	static native int expectationWorld(int[] world, int[] rankOrNull);
	static native int expectationCombine(double[] gatheredMoments4PerRankAndVector, int world, int count, double[] moments4PerVector);

	// ---- explicit fused programs: ops as parallel arrays {opcode, a, b, c, scalar}
	static native long programCreate(int[] opcode, int[] a, int[] b, int[] c, double[] scalar, int nInputs, int[] outValues, int[] reduceValues);
	static native int programRelease(long program);
	static native int programLaunchCount(long program, int[] launches);
	static native int programShape(long program, int[] inputsOutputsReductions3);
	static native int programRun(long program, int batch, long[] inputs, long[] outputs, double[] reduceShiftOrNull, double[] moments4OrNull, long deviceMomentsOrZero);
	static native int programRunInto(long program, int batch, long[] inputs, long[] outputs, double[] reduceShiftOrNull, double[] moments4OrNull, long deviceMomentsOrZero);

	// ---- execution tiers (replace JCudaUtils.preparePtxFile, JCudaUtils.java:37-122)
	static native int setJit(int mode, int[] previous);
	static native int jitWait();
	static native int jitStats(long[] compiledFailedPendingDiskHits, double[] compileSeconds);
	static native int programTier(long program, int[] tierAndVgprs);
	static native String programSource(int[] opcode, int[] a, int[] b, int[] c, double[] scalar, int nInputs, int[] outValues, int[] reduceValues);

	// ---- Brownian increments (replace curandGenerateNormal, BrownianMotionCudaWithRandomVariableCuda.java:168-178)
	static native int bmGenerate(long seed, int nSteps, int nFactors, long nPaths, long pathOffset, double[] dt, long[] outHandles);
	static native int mersenneIncrements(int seed, int nSteps, int nFactors, long nPaths, double[] dt, double[] hostOut);
	static native int bmGenerateMersenne(int seed, int nSteps, int nFactors, long nPaths, double[] dt, long[] outHandles);
	static native int bmGenerateMersenneDevice(int seed, int nSteps, int nFactors, long nPaths, long pathOffset, double[] dt, long[] outHandles);
	static native int incrementsHost(int seed, int nSteps, int nFactors, long nPaths, int[] kinds, double[] a, double[] b, double[] hostOut);
	static native int incrementsGenerateDevice(int seed, int nSteps, int nFactors, long nPaths, long pathOffset, int[] kinds, double[] a, double[] b, long[] outHandles);
	// quasi-Monte-Carlo: Sobol' points, the increments built from them on the host (the definition) and on the device (construction 0: increment by increment, 1: Brownian bridge)
	static native int sobolPointsHost(int nDims, long firstIndex, long count, int seed, int randomize, double[] uOut);
	static native int sobolIncrementsHost(int seed, int randomize, int construction, int nSteps, int nFactors, long nPaths, long pathOffset, double[] dt, double[] hostOut);
	static native int bmGenerateSobolDevice(int seed, int randomize, int construction, int nSteps, int nFactors, long nPaths, long pathOffset, double[] dt, long[] outHandles);
	static native double inverseNormalCdf(double p);

	// ---- pool (replace DeviceMemoryPool.clean / purge / getDeviceFreeMemPercentage, RandomVariableCuda.java:393-449)
	static native int poolClean();
	static native int poolPurge();
	static native int poolStats(long[] stats10);

	// ---- measurement
	static native int profileEnable(int enabled);
	static native int trafficStats(long[] algorithmicBytesAndSpecialisedLaunches);
	/** {size, kernelLaunches, specialisedLaunches, interpreterLaunches, algorithmicBytes, algorithmicBytesWritten, valuesDeferred, valuesDeferredNow, valuesDemanded, pendingOperations, peakBytesReserved,
	 *  lateReleasesWhileWaiting, lateReleasesAtOnce, lateReleaseNanoseconds, mergedLaunches, mergedChains, commonRows, rolledLaunches} */
	static native int engineStats(long[] stats18);
	static native int profileRead(double[] kernelMsTotal, long[] launches);

	// ---- helpers (plain Java)
	static long checkHandle(final long handle) {
		if(handle == 0) {
			throw new RuntimeException("fmhip: " + lastError());
		}
		return handle;
	}

	static void check(final int status) {
		if(status == 0) {
			return;
		}
		final String message = "fmhip error " + status + ": " + lastError();
		if(status == -3) {
			throw new OutOfMemoryError(message);					// as RandomVariableCuda.java:375
		}
		if(status == -7) {
			throw new UnsupportedOperationException(message);
		}
		throw new RuntimeException(message);
	}
}
