/*
 * fmhip.h — C-ABI of the MI355X-native RandomVariable / BrownianMotion engine.
 *
 * This is the drop-in boundary.  It replaces the JCuda/JCurand JNI surface
 * that the reference binds for this path:
 *
 *   reference (Java, JCuda)                                   this header
 *   ---------------------------------------------------------------------------------------------
 *   cuInit/cuDeviceGet/cuCtxCreate/cuModuleLoad               fmhip_init / fmhip_shutdown
 *     (RandomVariableCuda.java:159-248)
 *   DeviceMemoryPool.getDevicePointer(long)  (:280)           fmhip_vec_create_uninitialized
 *   DeviceMemoryPool.getDevicePointer(float[]) (:457)         fmhip_vec_create_from_float / _from_double
 *   DeviceMemoryPool.getValuesAsFloat        (:469)           fmhip_vec_read_float / _read_double
 *   DeviceMemoryPool.callFunctionv1s0 … v2s1 (:483-557)       fmhip_call_v1s0 … fmhip_call_v3s0
 *   DeviceMemoryPool.clean / purge           (:393,:424)      fmhip_pool_clean / fmhip_pool_purge
 *   getDeviceFreeMemPercentage               (:435)           fmhip_pool_stats
 *   getAverage/getVariance/getMin/getMax     (:830-901)       fmhip_reduce_moments (on device, 32 B back)
 *   curandCreateGenerator/SetSeed/GenerateNormal/Destroy      fmhip_bm_generate
 *     (BrownianMotionCudaWithRandomVariableCuda.java:141-182)
 *   — (no equivalent: one launch per method call)             fmhip_program_* (fused op streams, batched)
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = FMHIP_OK, <0 = error class);
 *     a human-readable message for the calling thread's last error is returned by fmhip_last_error().
 *   - a vector handle (fmhip_vec) is an opaque non-zero int64 owned by the caller; release it with
 *     fmhip_vec_release.  Storage is fp32 on the device (README.md:100 of the reference), values cross
 *     the boundary as double or float.
 *   - scalars are passed as double and narrowed with (float) before use, as the reference does
 *     (RandomVariableCuda.java:521,533).
 *   - all entry points are thread-safe; device work is enqueued on one in-order stream per engine — one engine per process
 *     (fmhip_init), per listed device (fmhip_init_devices) or per caller thread (fmhip_set_thread_engines); only the read /
 *     reduce entry points block.
 *   - a process drives one GPU (fmhip_init: one rank per GPU under torch.distributed / RCCL) or several (fmhip_init_devices).
 *   - a handle may be released late and from another thread (a garbage collector's cleaner: what the reference's WeakReference /
 *     ReferenceQueue pool and the Java binding's Cleaner do): the engine does not decide what to store by live handles, see
 *     fmhip_engine_stats.
 */
#ifndef FMHIP_H
#define FMHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMHIP_ABI_VERSION 1

typedef int64_t fmhip_vec;      /* 0 is never a valid handle */
typedef int64_t fmhip_program;  /* 0 is never a valid handle */

typedef enum fmhip_status {
    FMHIP_OK                  =  0,
    FMHIP_ERR_INVALID_HANDLE  = -1,
    FMHIP_ERR_SIZE_MISMATCH   = -2,
    FMHIP_ERR_OUT_OF_MEMORY   = -3,   /* maps to java.lang.OutOfMemoryError (RandomVariableCuda.java:375) */
    FMHIP_ERR_HIP             = -4,   /* a HIP runtime call failed (CudaException in the reference, :167) */
    FMHIP_ERR_INVALID_ARGUMENT= -5,
    FMHIP_ERR_NOT_INITIALIZED = -6,
    FMHIP_ERR_UNSUPPORTED     = -7,   /* UnsupportedOperationException in the reference */
    FMHIP_ERR_PROGRAM_LIMIT   = -8    /* a fused program exceeds the register / input budget */
} fmhip_status;

/*
 * Opcodes.  One per kernel of RandomVariableCudaKernel.cu (line numbers of the .cu given), plus the
 * operations the reference defines only in its CPU twin RandomVariableFromFloatArray.java
 * (choose :1264, isNaN :1441, sin :927, cos :942, addRatio :1395, subRatio :1418).
 * Arithmetic contract for every opcode: each elementary operation rounds to fp32 separately
 * (no FMA contraction — the reference compiles with `nvcc -fmad false`, JCudaUtils.java:69-70);
 * exp/log/pow/sin/cos are evaluated in fp64 and narrowed, sqrt and division are correctly rounded.
 */
typedef enum fmhip_opcode {
    /* vector (a) ∘ scalar (s):  fmhip_call_v1s1 */
    FMHIP_OP_CAP_S      =  1,  /* min(a,s)        capByScalar   .cu:2   */
    FMHIP_OP_FLOOR_S    =  2,  /* max(a,s)        floorByScalar .cu:13  */
    FMHIP_OP_ADD_S      =  3,  /* a + s           addScalar     .cu:24  */
    FMHIP_OP_SUB_S      =  4,  /* a - s           subScalar     .cu:34  */
    FMHIP_OP_BUS_S      =  5,  /* -a + s          busScalar     .cu:44  */
    FMHIP_OP_MULT_S     =  6,  /* a * s           multScalar    .cu:54  */
    FMHIP_OP_DIV_S      =  7,  /* a / s           divScalar     .cu:65  */
    FMHIP_OP_VID_S      =  8,  /* s / a           vidScalar     .cu:76  */
    FMHIP_OP_POW_S      =  9,  /* pow(a,s)        cuPow         .cu:98  */
    /* unary:  fmhip_call_v1s0 */
    FMHIP_OP_SQUARED    = 10,  /* a * a           squared       .cu:87  */
    FMHIP_OP_SQRT       = 11,  /* sqrt(a)         cuSqrt        .cu:109 */
    FMHIP_OP_EXP        = 12,  /* exp(a)          cuExp         .cu:119 */
    FMHIP_OP_LOG        = 13,  /* log(a)          cuLog         .cu:129 */
    FMHIP_OP_INVERT     = 14,  /* 1.0f / a        invert        .cu:139 */
    FMHIP_OP_ABS        = 15,  /* |a|             cuAbs         .cu:149 */
    FMHIP_OP_SIN        = 16,  /* sin(a)          twin :927     */
    FMHIP_OP_COS        = 17,  /* cos(a)          twin :942     */
    FMHIP_OP_ISNAN      = 18,  /* a!=a ? 1 : 0    twin :1441    */
    /* vector ∘ vector:  fmhip_call_v2s0 */
    FMHIP_OP_CAP        = 19,  /* min(a,b)        cap           .cu:160 */
    FMHIP_OP_FLOOR      = 20,  /* max(a,b)        cuFloor       .cu:170 */
    FMHIP_OP_ADD        = 21,  /* a + b           add           .cu:180 */
    FMHIP_OP_SUB        = 22,  /* a - b           sub           .cu:191 */
    FMHIP_OP_MULT       = 23,  /* a * b           mult          .cu:202 */
    FMHIP_OP_DIV        = 24,  /* a / b           cuDiv         .cu:213 */
    /* two vectors and a scalar:  fmhip_call_v2s1 */
    FMHIP_OP_ACCRUE     = 25,  /* a * (1 + b*s)   accrue        .cu:224 */
    FMHIP_OP_DISCOUNT   = 26,  /* a / (1 + b*s)   discount      .cu:234 */
    FMHIP_OP_ADDPRODUCT_VS = 27, /* a + b*s       addProduct_vs .cu:257 */
    /* three vectors:  fmhip_call_v3s0 */
    FMHIP_OP_ADDPRODUCT = 28,  /* a + b*c         addProduct    .cu:247 */
    FMHIP_OP_ADDRATIO   = 29,  /* a + b/c         addRatio      .cu:267 */
    FMHIP_OP_SUBRATIO   = 30,  /* a - b/c         subRatio      .cu:277 */
    FMHIP_OP_CHOOSE     = 31,  /* a>=0 ? b : c    twin :1264    */
    FMHIP_OP__COUNT     = 32
} fmhip_opcode;

/* Result of an on-device reduction over one vector (all fp64). */
typedef struct fmhip_moments {
    double sum;     /* Σ (x_i - shift)            */
    double sumsq;   /* Σ (x_i - shift)^2          */
    double min;     /* min x_i (NaN if any NaN, Java Math.min semantics) */
    double max;     /* max x_i (NaN if any NaN)   */
} fmhip_moments;

typedef struct fmhip_pool_stats_t {
    int64_t bytes_reserved;     /* device bytes obtained from hipMalloc and still held      */
    int64_t bytes_in_use;       /* bytes handed out to live vectors                         */
    int64_t bytes_cached;       /* bytes sitting in free lists                              */
    int64_t device_bytes_free;  /* hipMemGetInfo free (queried here only, never on the hot path) */
    int64_t device_bytes_total;
    int64_t n_alloc_hits;       /* allocations served from a free list                      */
    int64_t n_alloc_misses;     /* allocations that had to call hipMalloc                   */
    int64_t n_live_vectors;
    int64_t n_kernel_launches;  /* launches since init (fusion statistics)                  */
    int64_t n_ops_executed;     /* element-wise ops executed inside those launches          */
} fmhip_pool_stats_t;

/* ---------------------------------------------------------------- lifecycle */

/* Bind this process to one device and create the runtime (stream, pool, kernels).
 * device_index < 0: use env FMHIP_DEVICE_INDEX, else LOCAL_RANK, else 0.
 * Idempotent for the same device.  (RandomVariableCuda.java:159-248) */
int fmhip_init(int device_index);
/* ONE process, SEVERAL devices (replaces the single device index of RandomVariableCuda.java:161,177): every
 * vector is cut into contiguous blocks of paths (boundaries at multiples of four), block d lives on devices[d], every method runs on
 * every block, a read gathers the blocks by one device-to-host copy per device, and host-side moments are the per-device moments
 * added in device order (the rule of fmhip_expectation_combine) — no collective, nothing travels between devices.  Everything else of
 * this header works unchanged on the caller's side; handles are the library's own numbers.  An index may repeat (shards on separate
 * streams of one device: how this is tested on a one-GPU box).  Calls that only return handles are queued to one worker thread per
 * device and return at once: an error a device meets later (an allocation that fails) is returned by the next call that waits (a read,
 * a reduction, fmhip_synchronize).  Expectations wanted ON the devices — fmhip_reduce_moments_batch_devices: a buffer per listed
 * device; the *_device variants: a buffer on the first listed device — are the ONE exchange between the devices: every shard's launches
 * leave its moments in a device buffer of its own, one RCCL all-gather issued for all listed devices inside ncclGroupStart /
 * ncclGroupEnd makes every device hold all of them, a kernel per device combines them in device order (fmhip_expectation_combine's
 * rule: the same bits everywhere); with a repeated index — or without librccl.so, which is looked up at run time — they are combined
 * on the host instead (fmhip_expectation_collective tells which).  Not available with a device list: fmhip_get_stream (use
 * fmhip_get_stream_of), fmhip_vec_device_ptr, device_moments of fmhip_program_run, fmhip_set_expectation_comm with more than one
 * rank.  count == 1 is fmhip_init(devices[0]).  UNMEASURED on more than one physical GPU. */
int fmhip_init_devices(const int* devices, int count);
int fmhip_device_count(int* count);           /* devices (shards) behind the handles: 1 after fmhip_init */
/* An ENGINE PER CALLER THREAD on the one device of fmhip_init: every thread that calls into the library gets a pending graph, a stream,
 * a memory pool, a time-step grouping and a lock of its own (the thread that switches this on keeps the engine it initialised).  Threads
 * that simulate side by side — finmath-lib's optimiser evaluates the columns of a Jacobian on a thread pool
 * (LIBORMarketModelCalibrationATMTest.java:319) — record without meeting each other and their launches share the device.  Handles stay
 * valid everywhere: a vector of another thread is computed by ITS engine if it is still pending and enters a method as an operand that
 * aliases that storage (streams ordered by events); release, retain, read, moments, programs and tickets of another thread run on the
 * owner's engine.  Settings (fusion, math mode, JIT mode, step grouping) apply to every engine; fmhip_flush and fmhip_fusion_hold to the
 * calling thread's; statistics are summed; fmhip_synchronize waits for all.  Not together with a device list.  Ends with fmhip_shutdown.
 * Vectors are immutable, which is what makes sharing them safe; the two ways to WRITE into one (fmhip_program_run_into, a raw device pointer)
 * are the caller's to order against other threads' use of that vector (fmhip_synchronize).
 * The reference funnels every thread through one executor thread (RandomVariableCuda.java:155). */
int fmhip_set_thread_engines(int enabled, int* previous);
int fmhip_shutdown(void);
int fmhip_is_initialized(void);
int fmhip_abi_version(void);
/* Message of the calling thread's most recent failing call ("" if none). Never NULL. */
const char* fmhip_last_error(void);
/* Device name into buf (NUL-terminated, truncated), CU count, HBM bytes. Any pointer may be NULL. */
int fmhip_device_info(char* name_buf, int name_buf_len, int* n_compute_units, int64_t* hbm_bytes);
/* Block until all enqueued device work is complete (cuCtxSynchronize in the reference, :474). */
int fmhip_synchronize(void);
/* The HIP stream (hipStream_t as void*) all work is enqueued on — for interop with torch / RCCL. */
int fmhip_get_stream(void** stream_out);

/* ---------------------------------------------------------------- vectors */

/* Narrow double→float on the host (RandomVariableCuda.java:768-774) and upload. n >= 0. */
int fmhip_vec_create_from_double(const double* host_values, int64_t n, fmhip_vec* out);
int fmhip_vec_create_from_float(const float* host_values, int64_t n, fmhip_vec* out);
/* Device vector with every element = (float)value (twin ctor RandomVariableFromFloatArray.java:139-146). */
int fmhip_vec_create_filled(int64_t n, double value, fmhip_vec* out);
/* Pool allocation without initialisation (RandomVariableCuda.getDevicePointer(long), :737). */
int fmhip_vec_create_uninitialized(int64_t n, fmhip_vec* out);
int fmhip_vec_retain(fmhip_vec v);
int fmhip_vec_release(fmhip_vec v);
int fmhip_vec_size(fmhip_vec v, int64_t* n_out);
/* getRealizations(): materialise, D2H, widen float→double (RandomVariableCuda.java:1116-1123). */
int fmhip_vec_read_double(fmhip_vec v, double* host_out, int64_t n);
int fmhip_vec_read_float(fmhip_vec v, float* host_out, int64_t n);
/* Raw device pointer of the (materialised) fp32 storage; valid until the handle is released.  Vectors that were computed as identical
 * rows of one launch share their storage (the same inputs, the same scalars: computed once); a vector that shares it receives storage
 * of its own here, and in fmhip_program_run_into, before the pointer is handed out — writing through it never changes another vector. */
int fmhip_vec_device_ptr(fmhip_vec v, void** device_ptr_out);

/* ---------------------------------------------------------------- eager ops, one per reference launch helper */

/* result = f(a)            callFunctionv1s0 (RandomVariableCuda.java:483) */
int fmhip_call_v1s0(int opcode, fmhip_vec a, fmhip_vec* out);
/* result = f(a, (float)s)  callFunctionv1s1 (:515) */
int fmhip_call_v1s1(int opcode, fmhip_vec a, double s, fmhip_vec* out);
/* result = f(a, b)         callFunctionv2s0 (:493) */
int fmhip_call_v2s0(int opcode, fmhip_vec a, fmhip_vec b, fmhip_vec* out);
/* result = f(a, b, (float)s) callFunctionv2s1 (:527) */
int fmhip_call_v2s1(int opcode, fmhip_vec a, fmhip_vec b, double s, fmhip_vec* out);
/* result = f(a, b, c)      callFunctionv3s0 (:504) */
int fmhip_call_v3s0(int opcode, fmhip_vec a, fmhip_vec b, fmhip_vec c, fmhip_vec* out);

/* Deferred execution of the five calls above: when enabled they only record a node and return a
 * pending handle; chains are executed as ONE fused launch when a value is needed (read, reduce,
 * device_ptr, fmhip_flush) — results are bit-identical to eager execution. Default: disabled (eager).
 * Returns the previous setting through *previous (may be NULL). */
int fmhip_set_fusion(int enabled, int* previous);
/* Execute every pending node that is still referenced by a live handle (identical programs over
 * different vectors are batched into one launch). */
int fmhip_flush(void);
/* While held (hold != 0), a pending chain is never executed on the engine's own accord (normally it is once ≈ 40 methods
 * have accumulated below one handle, so that the device starts early); it runs when a value is needed or at fmhip_flush.
 * For callers that record many independent chains of identical structure — all products of a valuation, all bumped
 * parameter sets of a Jacobian — and want them batched as rows of the same launches.  Releasing the hold executes nothing
 * by itself.  hold == 2 is a SOFT hold: the same, except that everything pending is executed once more than 32768
 * operations wait — for helpers that group work on a caller's behalf and cannot know when the caller is done
 * (BrownianMotionHip groups the time steps of an Euler scheme this way).  Returns the previous setting (0, 1 or 2)
 * through *previous (may be NULL). */
int fmhip_fusion_hold(int hold, int* previous);
/* Time-step grouping on behalf of callers that give no hints (finmath-lib's Euler scheme through the RandomVariable interface).
 * A discretisation scheme reads the Brownian increments of time index i exactly while it computes step i; the engine watches for
 * the first use of an increment of fmhip_bm_generate with a new time index and keeps the methods recorded between `steps` such
 * boundaries pending (as under a soft hold), then executes them together — whole time steps, scheduled component by component,
 * their periodic stretch as one rolled-loop launch — instead of cutting the stream every ≈ 40 methods.  The last time index of a
 * generation ends the grouping.  Only while the fusion front-end is on and the caller holds nothing itself (fmhip_fusion_hold).
 * steps = 0 switches it off; default 4 (environment: FMHIP_GROUP_STEPS).  Results never depend on it.
 * Replaces what BrownianMotionCudaWithRandomVariableCuda's callers get from the reference: nothing (one launch per method).
 * Returns the previous setting through *previous (may be NULL). */
int fmhip_set_step_grouping(int steps, int* previous);
/* Replicate PENDING expressions: a caller that is about to record the same chain of methods again with other vectors and other
 * scalar operands — the next scenario, the next bumped parameter set of a Jacobian — records it ONCE and asks for copies.
 * The graph = every pending (not yet executed) operation below `roots`.  Copy j reads leaf_to[j*n_map + i] wherever the
 * original reads leaf_from[i] (operands outside the graph; operands not listed are shared by all copies), and takes its scalar
 * operands from scalars[j*n_scalars + k], k counting the graph's scalar-carrying operations in the order they were recorded
 * (scalars == NULL: the original's; otherwise n_scalars must equal the graph's count — see fmhip_graph_scalars).
 * out[j*n_roots + r] receives the copy of roots[r] (a handle the caller releases); the inner values of a copy have no handle.
 * Cost ≈ 50 ns per operation and copy, against one C call, one handle and one release per operation when recorded by hand.
 * The copies are ordinary pending expressions: the next flush batches them with the original as rows of the same launches.
 * Requires the fusion front-end (fmhip_set_fusion); results are bit-identical to recording each copy by hand. */
int fmhip_graph_clone(const fmhip_vec* roots, int n_roots, int n_copies,
                      const fmhip_vec* leaf_from, const fmhip_vec* leaf_to, int n_map,
                      const double* scalars, int n_scalars, fmhip_vec* out);
/* The scalar operands of the pending graph below `roots`, in recording order: *n_scalars receives their number, the first
 * min(capacity, number) go to scalars_out (may be NULL).  Lets a caller check its scalar list against what it recorded. */
int fmhip_graph_scalars(const fmhip_vec* roots, int n_roots, double* scalars_out, int capacity, int* n_scalars);

/* Arithmetic mode of exp and log (everything else is identical in both modes):
 *   FMHIP_MATH_EXACT (default): evaluated in fp64 and narrowed once — bit-identical to the reference's CPU twin
 *                               `(float)Math.exp(x)` except where two fp64 libms differ in the last fp64 ulp;
 *   FMHIP_MATH_FAST:            hardware v_exp_f32 / v_log_f32 with fp32 range reduction, within 2 fp32 ulp — the accuracy
 *                               class of the CUDA expf/logf used by the reference's kernels; ~4x fewer instructions.
 * Applies to programs compiled after the call (eager ops, fused chains, fmhip_program_create). */
#define FMHIP_MATH_EXACT 0
#define FMHIP_MATH_FAST  1
int fmhip_set_math_mode(int mode, int* previous);

/* ---------------------------------------------------------------- reductions */

/* One pass over v on the device: Σ(x-shift), Σ(x-shift)², min, max with fp64 accumulation; 32 bytes
 * come back.  Replaces the reference's D2H of the whole vector + host loops
 * (RandomVariableCuda.java:830-901 → RandomVariableFromFloatArray.java:284-382).
 * The moments of a vector are a function of its elements and its length alone (one reduction tree per vector): the same bits
 * whether a launch of their own computes them, the launch that computes the vector, or a launch over many vectors.  With fusion
 * on (fmhip_set_fusion) and v pending among much other pending work, the call may execute ALL pending work — expressions of equal
 * shape as rows of the same launches — and keep the unshifted moments of every vector those launches produce: later calls for
 * those vectors return them without a launch (vectors are immutable; fmhip_program_run_into and fmhip_vec_device_ptr make the
 * engine forget).  Never under the caller's hard hold (fmhip_fusion_hold(1)).  The calling thread waits for the device without
 * holding the engine: other threads keep recording and launching. */
int fmhip_reduce_moments(fmhip_vec v, double shift, fmhip_moments* out);
/* Same, but the 4 doubles are written to caller-owned DEVICE memory (e.g. a torch tensor that is then
 * all-reduced with RCCL); asynchronous on the runtime stream. */
int fmhip_reduce_moments_device(fmhip_vec v, double shift, void* device_out_4_doubles);

/* `count` vectors of equal size reduced by ONE launch and one 32·count-byte read-back (all expectations of one objective
 * evaluation at once).  shifts may be NULL (= 0 for all). */
int fmhip_reduce_moments_batch(const fmhip_vec* vectors, int count, const double* shifts, fmhip_moments* out);
/* Same, results (count x 4 doubles) left in caller-owned DEVICE memory, asynchronous on the runtime stream — the send buffer
 * of the one RCCL all-reduce per objective evaluation when paths are sharded over GPUs. */
int fmhip_reduce_moments_batch_device(const fmhip_vec* vectors, int count, const double* shifts, void* device_out);
/* The same ON EVERY DEVICE of a device list (fmhip_init_devices): device_out[d] — a buffer of count x 32 bytes on the d-th listed device,
 * the caller's own allocation; NULL: not wanted there — receives the moments of the WHOLE vectors, all path shards combined in device
 * order (bit-identical on every device).  Nothing is waited for: the result is ordered on the shards' streams (fmhip_get_stream_of).
 * n_devices = fmhip_device_count (with one device: 1, and this is fmhip_reduce_moments_batch_device).  The reference has no counterpart
 * (one device index: RandomVariableCuda.java:161,177); SURVEY.md §8e. */
int fmhip_reduce_moments_batch_devices(const fmhip_vec* vectors, int count, const double* shifts, void* const* device_out, int n_devices);
/* The stream the work of device shard `shard` is ordered on (shard 0 of one device: fmhip_get_stream). */
int fmhip_get_stream_of(int shard, void** stream_out);
/* How expectations wanted on the devices of a device list travel: kind 0 = one device, nothing to exchange; 1 = a grouped RCCL all-gather
 * over the listed devices; 2 = combined on the host (`why`, if given, says why: a repeated device index, librccl.so not found …). */
int fmhip_expectation_collective(int* kind, char* why, int why_len);
/* The same reduction in two halves: _begin enqueues it and returns a ticket at once; _end waits for THAT reduction — not for work
 * enqueued after it — writes the `count` moments (the expectation communicator applied, as in fmhip_reduce_moments_batch) and
 * retires the ticket.  A caller that evaluates one parameter set after the other records and enqueues set k+1 between the two
 * halves of set k: the device never waits for the host at the boundary (one in-order stream: a blocking read of set k's results
 * AFTER set k+1 was enqueued would wait for set k+1 as well).  The reference has no counterpart: its getAverage() synchronises
 * the context (RandomVariableCuda.java:869-878).  A ticket must be ended exactly once. */
typedef int64_t fmhip_ticket;
int fmhip_reduce_moments_batch_begin(const fmhip_vec* vectors, int count, const double* shifts, fmhip_ticket* ticket_out);
int fmhip_reduce_moments_batch_end(fmhip_ticket ticket, fmhip_moments* out, int count);
/* For a caller that wants the EXPECTATIONS of vectors and will never read their values — a Monte-Carlo product's payoff, of which
 * getValue() returns the average.  A vector that is still a pending expression and that only the caller references need then not be
 * written to memory at all: when a later fmhip_reduce_moments / _batch / _batch_begin runs what is pending, the launch that computes
 * such a vector takes its moments and drops it (the one store per workgroup behind a chain of reads costs that launch 8-10 % of its
 * rate).  After this call the values of `vectors` must not be read or used as operands again
 * (FMHIP_ERR_INVALID_ARGUMENT where the engine has in fact not kept them); their moments stay available; the handles are released
 * as usual.  Vectors computed already, or referenced by somebody else, are simply left as they are.  The reference has no
 * counterpart: its getAverage() copies the whole vector to the host (RandomVariableCuda.java:869-878). */
int fmhip_vec_give_up_values(const fmhip_vec* vectors, int count);

/* Order statistics on the device: what getQuantile, getQuantileExpectation and getHistogram need, without the vector
 * leaving the device and without a sort (the reference downloads and sorts: RandomVariableCuda.java:970-1091).  The order is that of
 * java.util.Arrays.sort(float[]): -0.0 before +0.0, every NaN equal and last.  RANKS cross this boundary, not quantiles: the index formula
 * (and its rounding rule) stays with the caller.  All vectors of a batch have the same size n > 0; pending vectors are computed (one flush
 * for the batch); a vector whose values were given up (fmhip_vec_give_up_values) is the error a read of it is.  Arguments are checked on
 * the host before anything is launched: a rank outside [0, n), n == 0, count or n_ranks < 1 -> FMHIP_ERR_INVALID_ARGUMENT; vectors of
 * different sizes -> FMHIP_ERR_SIZE_MISMATCH.  A selected value is an element of the vector: the answers are those of the sort, bit for bit.
 * With a device list the shards' counts are added by the library; with an expectation communicator (below) the results are those of the
 * GLOBAL sample of world*n elements on every rank — ranks in [0, world*n), one gather per pass, sums added in rank order.
 *
 * fmhip_select_ranks_batch: values_out[k*n_ranks + j] = sorted(vectors[k])[ranks[j]] as double (NaN for a position in the NaN tail).
 *   A radix select of four 8-bit passes; count x n_ranks (vector, rank) pairs share the passes: four launches per eight ranks, whatever `count`.
 * fmhip_rank_sums_batch: sums_out[k] = sum of sorted(vectors[k])[rank_from .. rank_to] (both inclusive, from <= to) in fp64: the two ends
 *   selected as above, ties at the ends multiplied, the elements strictly between added in an order that depends on n alone.  A range that
 *   reaches the NaN tail, or holds +inf and -inf, sums to NaN.
 * fmhip_count_not_above: counts_out[j] = #{ i : (double)v[i] <= bounds[j] } (the comparison of the reference's histogram loop); NaN
 *   elements are never counted, a NaN bound counts nothing; bounds in any order, any number of them (4096 per launch). */
int fmhip_select_ranks_batch(const fmhip_vec* vectors, int count, const int64_t* ranks, int n_ranks, double* values_out);
int fmhip_rank_sums_batch(const fmhip_vec* vectors, int count, int64_t rank_from, int64_t rank_to, double* sums_out);
int fmhip_count_not_above(fmhip_vec v, const double* bounds, int n_bounds, int64_t* counts_out);

/* Cross moments: the normal equations of a least-squares regression in one pass over the data — what finmath-lib's
 * MonteCarloConditionalExpectationRegression assembles from b_i.mult(b_j).getAverage(), product by product.  n_x vectors x (1 … 12) and
 * n_y vectors y (0 … 4), all of one size n > 0; a handle of 0 among x stands for the constant 1 (it is not loaded), so the same pass also
 * yields the sums of the x_j and n itself: a regression with an intercept, a covariance.  The same handle may appear several times and in
 * both lists.  Every product of two fp32 values is exact in fp64 and is added in fp64; the order of the additions of one pair depends on n
 * alone, so the bits of a sum do not depend on how many other vectors the call names, on the roles (x or y) or on the positions.
 * sums_out: n_x(n_x+1)/2 doubles (S, upper triangle, row-major: (0,0) (0,1) … (0,n_x-1) (1,1) …) followed by n_x*n_y doubles (T[i*n_y + m]).
 * SUMS, not averages: shards and ranks add.  With a device list the library adds the shards' sums in shard order; with an expectation
 * communicator (below) every rank receives the sums of the GLOBAL sample (one gather, added in rank order).
 * Arguments are checked on the host before anything is launched: counts out of range, a NULL pointer, a 0 among y, no vector among x or
 * n == 0 -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  Pending vectors
 * are computed in one flush for the call, ONE kernel launch follows; a vector whose values were given up (fmhip_vec_give_up_values) is the
 * error a read of it is.  IEEE semantics: a NaN in x_3 makes exactly the entries that involve x_3 NaN, inf*0 is NaN. */
int fmhip_cross_moments(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out);

/* Wide cross moments: the same normal equations for n_x >= 1 vectors x and n_y >= 0 vectors y with n_x + n_y <= 64, in one
 * pass on the matrix cores (v_mfma_f64_16x16x4_f64) — a Longstaff-Schwartz basis on several underlyings, a covariance matrix of 63 vectors.
 * Output layout, the handle-0 constant 1 among x, status codes, the checks on the host before anything is flushed or launched and the IEEE
 * behaviour (a NaN in x_3 poisons exactly the entries with x_3; inf*0 is NaN) are exactly those of fmhip_cross_moments.
 * Every product of two fp32 values is exact in fp64 and is added in fp64; no float atomics, no fp32 product.  The bits of one pair's sum
 * are a function of n and of the two vectors' values only: not of how many vectors the call names, of where in the lists the two stand, of
 * which of the two comes first, or of whether the pair is reported in S or in T.  They need not equal fmhip_cross_moments' bits for the
 * same pair (the tree is another one; the longest chain of additions is xmom_wide_chain(n), csrc/xmom_wide_kernel.h, and the sums agree
 * with any summation order's to (chain + 1)*2^-53*sum|terms|).  ONE launch.  A build without the kernel answers FMHIP_ERR_UNSUPPORTED; it
 * never falls back.  Device lists add in shard order; an expectation communicator does one gather, added in rank order. */
int fmhip_cross_moments_wide(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out);

/* Localized regression: the cross moments above PER BIN of a key vector — the block-diagonal normal equations of a
 * regression that is local in the key (finmath-lib: BermudanOption's binning basis, the ...LocalizedOnDependentRegression estimators) — in
 * one pass, and the piecewise estimate as a new vector.
 * Bins: bounds[n_bins - 1] doubles, non-decreasing, +-inf allowed, 1 <= n_bins <= 64 (bounds may be NULL for one bin).
 *   bin(k) = #{ j : bounds[j] < (double)k }: k lies in bin j iff bounds[j-1] < k <= bounds[j] — the comparison of fmhip_count_not_above, so
 *   -0.0 and +0.0 fall on the same side of a bound of 0.  A NaN key belongs to no bin.
 * fmhip_binned_cross_moments: n_x vectors x (1 ... 3; a handle of 0 is the constant 1 and is not loaded) and n_y vectors y (0 ... 4), all of
 *   the key's size n > 0.  counts_out[n_bins]: the paths per bin.  sums_out[n_bins][q], q = n_x(n_x+1)/2 + n_x*n_y: per bin the fp64 SUMS in
 *   the layout of fmhip_cross_moments (S packed upper triangle, then T).  Every product of two fp32 values is exact in fp64 and is added in
 *   fp64; no float atomics.  The bits of one (bin, pair) sum are a function of n, of which path positions fall into that bin and of the two
 *   vectors' values there — not of the other vectors the call names, of list order or role, or of the bounds of other bins (they need not
 *   equal fmhip_cross_moments' bits at n_bins = 1).  ONE launch.
 * fmhip_binned_evaluate: *out = a new, materialised vector r with r[p] = ((x_0[p]*c_0) + x_1[p]*c_1) + x_2[p]*c_2,
 *   c_i = (float)coefficients[bin(key[p])*n_x + i]: every product and every sum rounded to fp32, nothing contracted — what
 *   basis[0].mult(b0).addProduct(basis[i], bi) computes with that bin's coefficients.  The constant 1 is 1.0f; a NaN key gives NaN.  Eager:
 *   pending operands are computed in one flush, one launch follows.
 * The _host functions are the DEFINITION over host float arrays (a NULL among x is the constant 1) and need no device; a bin's members are
 *   added in path order there.  The device's sums agree with any summation order's to count*2^-53*sum|terms| per bin.
 * Everything is checked on the host before anything is flushed or launched, by one function for the device and the host entry point:
 * counts out of range, a NULL pointer, unsorted bounds, a NaN bound, a 0 among y or as the key, n == 0 -> FMHIP_ERR_INVALID_ARGUMENT;
 * vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read
 * of it is.  A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.  With a device list counts and sums add in shard
 * order and the evaluation is per shard; with an expectation communicator counts and sums are those of the GLOBAL sample (one gather, added
 * in rank order). */
int fmhip_binned_cross_moments(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y,
                               int64_t* counts_out, double* sums_out);
int fmhip_binned_cross_moments_host(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x,
                                    const float* const* y, int n_y, int64_t* counts_out, double* sums_out);
int fmhip_binned_evaluate(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const double* coefficients, fmhip_vec* out);
int fmhip_binned_evaluate_host(const float* key, int64_t n, const double* bounds, int n_bins, const float* const* x, int n_x,
                               const double* coefficients, float* out);

/* Sort on the device: the whole ordered sample, the permutation and the ranks per path without the vector leaving the
 * device — what the reference downloads and sorts for.  A stable radix sort of (key, path index) pairs.
 * Order: ascending in the 32-bit key of the order statistics — the order of java.util.Arrays.sort(float[]):
 *   -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, every NaN (either sign, any payload) one key.  TIES ARE BROKEN BY PATH INDEX: equal keys
 *   keep ascending path order, NaNs among them.  Midranks (average ranks for ties) and descending order are not offered.
 * fmhip_sort_by_key: the key vector and n_values (0 ... 8) companion vectors of its size n (1 ... 2^31 - 1), reordered by the key's
 *   permutation: *sorted_key_out and sorted_values_out[i] are new, materialised vectors with out[r] = in[permutation[r]], copied BIT FOR BIT
 *   from the inputs (a NaN keeps its payload, a zero its sign).  sorted_key_out may be NULL when n_values > 0 (only the companions are
 *   wanted); the key may be among the companions.  The inputs are unchanged.
 * fmhip_argsort: permutation_out[n] on the host: permutation_out[r] = the path at position r of the ascending sample.
 * fmhip_argsort_host: the DEFINITION over a host float array; needs no device.
 * fmhip_rank_scores: *out = a new, materialised vector with out[p] = (float)((rank(p) + 0.5) / n), the quotient in fp64, rank(p) the ORDINAL
 *   rank of path p (the position of p in the permutation: ties by path index) — empirical-CDF scores strictly inside (0, 1).
 * fmhip_vec_read_elements: out[j] = (double)v[positions[j]] for count >= 1 positions in [0, n), in any order, repeats allowed: a few
 *   elements of a vector (the quantiles of a sorted one) without reading the vector.
 * Everything is checked on the host before anything is flushed or launched, with the status codes of the other passes: n_values outside
 * 0 ... 8, a NULL pointer, a handle of 0, nothing asked for, a position outside [0, n), n == 0 or n > 2^31 - 1 -> FMHIP_ERR_INVALID_ARGUMENT;
 * vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read
 * of it is.  A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.
 * ONE sample on ONE device: a global order needs an exchange of elements between devices, which is not done.  With a device list of more
 * than one shard, and with an expectation communicator of more than one rank, the three sorting calls answer FMHIP_ERR_UNSUPPORTED (never
 * the order of a part); fmhip_vec_read_elements answers FMHIP_ERR_UNSUPPORTED with a device list of more than one shard and reads this
 * rank's vector under a communicator. */
int fmhip_sort_by_key(fmhip_vec key, const fmhip_vec* values, int n_values, fmhip_vec* sorted_key_out, fmhip_vec* sorted_values_out);
int fmhip_argsort(fmhip_vec key, int64_t* permutation_out);
int fmhip_argsort_host(const float* key, int64_t n, int64_t* permutation_out);
int fmhip_rank_scores(fmhip_vec key, fmhip_vec* out);
int fmhip_vec_read_elements(fmhip_vec v, const int64_t* positions, int count, double* out);

/* Prefix sums on the device: the running sum along the sample without the vector leaving the device — the cumulative
 * weight behind a weighted quantile or a weighted expected shortfall, the expected-shortfall curve of a sorted loss vector, the running
 * average of an estimator against the number of paths.
 * P[r] is the fp64 sum of (double)v[0..r] in ONE association, a function of n and r alone (csrc/prefix_host.hpp): nested units — a lane's 8
 *   elements, the 8 lanes of a group, the 8 groups of a wave, the 4 waves of a tile, the tiles of a chunk, the chunks — in each of which the
 *   first subunit takes no base (it is not added to 0: a leading -0.0 stays -0.0) and every prefix of subunit j is fl(base + prefix inside),
 *   the base being the last prefix of subunit j - 1.  The device's P[r] EQUALS fmhip_prefix_sums_host's bit for bit in all three calls (of a
 *   NaN only that it is one).  For input without negative elements or NaNs P is non-decreasing.
 *   |P[r] - exact| <= (prefix_chain(n) + 1) * 2^-53 * sum_{i<=r} |v[i]|.
 * fmhip_prefix_sums: *out = a new, materialised vector of v's size n (1 ... 2^31 - 1): out[r] = (float)P[r], or with FMHIP_PREFIX_MEAN
 *   (float)(P[r] / (double)(r + 1)), the quotient the correctly rounded fp64 one.  total_out may be NULL and receives P[n-1].
 * fmhip_prefix_sums_at: sums_out[j] = P[positions[j]] in fp64 for count = 1 ... 4096 positions in [0, n), in any order, repeats allowed.  The
 *   vector is read once (and one chunk of it again per position); no output vector is written.
 * fmhip_prefix_search: positions_out[j] = the smallest r with P[r] >= t_j and sums_out[j] = that P[r]; if no r qualifies, n and P[n-1].
 *   t_j = thresholds[j], or fl(thresholds[j] * P[n-1]) in fp64 when relative != 0; count = 1 ... 4096.  A NaN prefix never qualifies and a NaN
 *   threshold finds nothing.  Defined for signed input too (P need not be monotone: the FIRST crossing is found).  total_out may be NULL
 *   and receives P[n-1].
 * fmhip_prefix_sums_host: the DEFINITION over a host float array: prefix_out[r] = P[r]; needs no device.
 * Everything is checked on the host before anything is flushed or launched, with the status codes of the other passes: a mode that is
 * neither, count outside 1 ... 4096, a NULL pointer, a handle of 0, a position outside [0, n), n == 0 or n > 2^31 - 1 ->
 * FMHIP_ERR_INVALID_ARGUMENT; FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of
 * it is.  A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.
 * ONE sample on ONE device: a carry between devices is not built.  With a device list of more than one shard, and with an expectation
 * communicator of more than one rank, the three device calls answer FMHIP_ERR_UNSUPPORTED (never the prefix sums of a part). */
#define FMHIP_PREFIX_SUM  0   /* out[r] = (float)P[r]                         */
#define FMHIP_PREFIX_MEAN 1   /* out[r] = (float)(P[r] / (double)(r + 1))     */
int fmhip_prefix_sums(fmhip_vec v, int mode, fmhip_vec* out, double* total_out);
int fmhip_prefix_sums_at(fmhip_vec v, const int64_t* positions, int count, double* sums_out);
int fmhip_prefix_search(fmhip_vec v, const double* thresholds, int count, int relative,
                        int64_t* positions_out, double* sums_out, double* total_out);
int fmhip_prefix_sums_host(const float* v, int64_t n, double* prefix_out);   /* the DEFINITION */

/* Resampling on the device: the step that follows the weighted sample of the prefix sums — the weighted sample becomes an
 * equally weighted one without a vector leaving the device: m ancestors a_j are drawn from the weights and up to 8 state vectors are
 * carried along, values_out[i][j] = values[i][a_j].  A particle filter's resampling step, importance sampling with weight degeneracy, the
 * bootstrap (weights == 0: equal weights), one draw of ancestors for several state vectors.  The definition is csrc/resample_host.hpp, one
 * header for the host and the device; fp64, every operation rounded on its own, no libm.
 *   cleaned weights  cw[r] = w[r] if w[r] > 0, otherwise +0.0: a NaN, a negative weight and -0.0 count as zero.
 *   P, total         P = fmhip_prefix_sums_host's P of cw (the same association, non-decreasing), total = P[n-1].  With weights == 0
 *                    P[r] = (double)(r + 1) and total = (double)n exactly: nothing is summed and nothing is searched.
 *   degenerate total !(total > 0) or total == +inf: every element of every output is the quiet NaN 0x7fc00000, the ancestors are NaN on the
 *                    device and -1 in the host twin, and the status is still FMHIP_OK (no data-dependent status); total_out tells.
 *   fraction f_j     FMHIP_RESAMPLE_SYSTEMATIC ((double)j + offset) / (double)m with ONE offset in [0, 1); _STRATIFIED ((double)j + U_j) /
 *                    (double)m; _MULTINOMIAL U_j (in the order of the uniforms: no sort is needed or done).  U_j = (double)uniforms[j]; below 0
 *                    it is taken as 0, at or above 1 as the largest double below 1; a NaN makes element j dead (NaN in every output).
 *   target, ancestor t_j = fl(f_j * total); a_j = the smallest r with P[r] > t_j, and if there is none (only rounding at the top can cause
 *                    that) the smallest r with P[r] == total.  Hence cw[a_j] > 0 ALWAYS — a path of zero weight is never an ancestor, at
 *                    t = 0 as little as anywhere — and 0 <= a_j <= n - 1 ALWAYS.  With equal weights a_j = min((int64)t_j, n - 1).
 *   outputs          values_out[i] = a new, materialised vector of m elements, copied bit for bit (a NaN keeps its payload, a zero its sign);
 *                    *ancestors_out (optional, n <= 2^24, where the float is exact) = (float)a_j.  The inputs are unchanged.
 * n is the size of weights, or of values[0] when weights is 0.  The device's bits are fmhip_resample_host's.
 * Checked on the host before anything is flushed or launched: an unknown scheme, m or n outside 1 ... 2^31 - 1, n_values outside 0 ... 8,
 * nothing asked for (n_values == 0 and no ancestors_out), neither weights nor a value vector, an offset outside [0, 1) or not finite
 * (whatever the scheme: pass 0 where it is not read), uniforms == 0 with a scheme that needs them (with _SYSTEMATIC they are not looked at),
 * ancestors_out with n > 2^24, a NULL pointer -> FMHIP_ERR_INVALID_ARGUMENT; a value vector whose size is not n, uniforms whose size is not
 * m -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A refusal leaves the outputs untouched and no vector behind.  A vector whose
 * values were given up is the error a read of it is.  If the pool cannot give the temporary of P (8n bytes): FMHIP_ERR_OUT_OF_MEMORY.  A
 * build without the kernel answers FMHIP_ERR_UNSUPPORTED; it never falls back.
 * ONE sample on ONE device, as the prefix sums: a device list of more than one shard or an expectation communicator of more than one rank
 * -> FMHIP_ERR_UNSUPPORTED. */
#define FMHIP_RESAMPLE_SYSTEMATIC  0
#define FMHIP_RESAMPLE_STRATIFIED  1
#define FMHIP_RESAMPLE_MULTINOMIAL 2
int fmhip_resample(fmhip_vec weights /* 0: equal weights */, int scheme, int64_t m, double offset,
                   fmhip_vec uniforms /* m elements; 0 with SYSTEMATIC */,
                   const fmhip_vec* values, int n_values /* 0 ... 8 */, fmhip_vec* values_out,
                   fmhip_vec* ancestors_out /* may be NULL */, double* total_out /* may be NULL */);
int fmhip_resample_host(const float* weights, int64_t n, int scheme, int64_t m, double offset, const float* uniforms,
                        const float* const* values, int n_values, float* const* values_out,
                        int64_t* ancestors_out, double* total_out);          /* the DEFINITION; needs no device */

/* Selection on the device: keep the paths on which a condition holds — copy_if —, put them back, and read by a caller's
 * index.  Longstaff-Schwartz on the in-the-money paths, a quantile or a tail mean given a barrier hit or a default, rare events whose
 * downstream work should run on 1 % of the paths, particles that are killed, one index list carried to any number of vectors.  The
 * definition is csrc/select_host.hpp, one header for the host and the device; counts are integers, nothing is summed in floating point:
 * the device's bits are the _host twins' for every input.
 *   selected(x)      x >= 0.0f in fp32, the trigger of FMHIP_OP_CHOOSE: a NaN is not selected, -0.0 is, +inf is.
 *   q(r), count      q(r) = the number of selected elements of mask before r; count = the number of all of them.
 *   fmhip_compress   for the selected r in ascending order: values_out[i][q(r)] = values[i][r] bit for bit (a NaN keeps its payload) and
 *                    positions_out[q(r)] = (float)r — new, materialised vectors of exactly `count` elements.  n_values is 0 ... 8;
 *                    values_out (with n_values == 0) and positions_out may be NULL; a call that only wants count_out is valid.  Positions
 *                    are offered up to n = 2^24, where the float is exact.  count == 0: FMHIP_OK, *count_out = 0, every output handle is
 *                    written as 0 and nothing is allocated — an empty vector is not a vector here.
 *   fmhip_expand     the inverse: values_out[i][r] = values[i][q(r)] where selected(mask[r]), otherwise (float)fill (which may be +-inf or
 *                    NaN) — new vectors of n elements.  n_values is 1 ... 8.  Every values[i] has exactly count(mask) elements, otherwise
 *                    FMHIP_ERR_SIZE_MISMATCH: found after the count, with no vector and no byte left behind.
 *   fmhip_gather     index has m elements, the values n each: values_out[i][j] = values[i][k] bit for bit where index[j] is an integer k
 *                    with 0 <= k <= n - 1 (-0.0 counts as 0; the comparison is made in double, so it is right for every n); anywhere else
 *                    — not an integer, out of range, NaN — the quiet NaN 0x7fc00000.  The status is FMHIP_OK whatever the index holds.
 *                    n_values is 1 ... 8.  gather(positions_out of a compress, v) is that compress of v.
 * compress and expand run in TWO phases with one host wait between them: the count is on the device, and the outputs are allocated at
 * exactly the size it says (a 1 % selection holds 1 % of the memory).  A refusal or a failed allocation at either stage leaves the outputs
 * untouched and no vector behind.
 * Checked on the host before anything is flushed or launched: n_values outside its range, nothing asked for, a handle of 0, a NULL pointer,
 * n or m outside 1 ... 2^31 - 1, positions_out with n > 2^24 -> FMHIP_ERR_INVALID_ARGUMENT; values whose size is not the mask's (compress)
 * or that differ among themselves -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A build without the kernels answers
 * FMHIP_ERR_UNSUPPORTED; it never falls back.
 * ONE sample on ONE device: a device list of more than one shard or an expectation communicator of more than one rank ->
 * FMHIP_ERR_UNSUPPORTED for all three (the shards' counts differ and an exchange between shards is not built).
 * The _host twins are the definitions on plain arrays and need no device.  fmhip_compress_host: values_out[i] and positions_out have
 * capacity n, the first *count_out elements are written; fmhip_expand_host: values[i] has n_value_elements elements, which must be the
 * mask's count (FMHIP_ERR_SIZE_MISMATCH, nothing written); fmhip_gather_host: index and values_out[i] have m elements, values[i] n. */
int fmhip_compress(fmhip_vec mask, const fmhip_vec* values, int n_values /* 0 ... 8 */, fmhip_vec* values_out,
                   fmhip_vec* positions_out /* may be NULL */, int64_t* count_out /* may be NULL */);
int fmhip_expand(fmhip_vec mask, const fmhip_vec* values, int n_values /* 1 ... 8 */, double fill, fmhip_vec* values_out);
int fmhip_gather(fmhip_vec index, const fmhip_vec* values, int n_values /* 1 ... 8 */, fmhip_vec* values_out);
int fmhip_compress_host(const float* mask, int64_t n, const float* const* values, int n_values, float* const* values_out,
                        int64_t* positions_out, int64_t* count_out);         /* the DEFINITION; needs no device */
int fmhip_expand_host(const float* mask, int64_t n, const float* const* values, int n_values, int64_t n_value_elements, double fill,
                      float* const* values_out);                             /* the DEFINITION */
int fmhip_gather_host(const float* index, int64_t m, const float* const* values, int n_values, int64_t n,
                      float* const* values_out);                             /* the DEFINITION */

/* Reduce by key on the device: out[k] = the sum of { v[j] : index[j] == k } — reduce_by_key, index_add, bincount with
 * weights — for an index vector that another pass left on the device: the ancestors of a resample (offspring counts), the slot of an
 * argmax, a bin number, a Poisson count (E[y | discrete state]), inner paths of unequal number, histograms of any number of bins.  The
 * definition is csrc/group_host.hpp, one header for the host and the device: the device's bits are the _host twin's for every input.
 *   membership       index[j] belongs to group k where it is the integer k with 0 <= k <= m - 1 (-0.0 counts as 0); anywhere else — NaN,
 *                    +-inf, a fraction, negative, >= m — the element belongs to NO group and is counted in *ungrouped_out.  The status is
 *                    FMHIP_OK whatever the index holds.  m is 1 ... 2^24, where the float index is exact.
 *   the sums         the members of a group are summed in ascending path order, in fp64, as the run-prefixes of the prefix sums' tree over
 *                    the elements ordered by (group, path): S1 of (double)v, S2 of the exact squares.  With one group S1 is P[n - 1] of
 *                    fmhip_prefix_sums_host bit for bit; a group of one member is that member; the bits of a group do not depend on the
 *                    values of other groups, on n_values, on a vector's slot or on the mask; |S - exact| <= (chain(n) + 1) 2^-53 times the
 *                    sum of the |terms| of that group alone.  A NaN or +-inf stays inside its own group.
 *   outputs          new, materialised vectors of m elements, rounded to fp32 once: *counts_out the count as a float (may be NULL); outs,
 *                    n_values x popcount(mask) handles, vector-major, the mask's bits ascending: FMHIP_BLOCK_SUM (float)S1, FMHIP_BLOCK_MEAN
 *                    (float)(S1 / count), FMHIP_BLOCK_VARIANCE (float)max(0, S2/count - (S1/count)^2), the population variance from raw
 *                    moments with the caveat of fmhip_block_moments.  An EMPTY group has count 0, sum +0.0, mean and variance NaN
 *                    (0x7fc00000, as every NaN that comes back).
 * n_values is 0 ... 4: a call with none asks for counts_out or ungrouped_out (or both).
 * Checked on the host before anything is flushed or launched: m or n_values outside their range, a mask of 0 with n_values > 0, a mask
 * with unknown bits, nothing asked for, a handle of 0, a NULL pointer -> FMHIP_ERR_INVALID_ARGUMENT; values whose size is not the index's
 * -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A refusal or a failed allocation at any stage leaves the outputs untouched and no
 * vector behind.  A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.
 * ONE sample on ONE device: a device list of more than one shard or an expectation communicator of more than one rank ->
 * FMHIP_ERR_UNSUPPORTED.
 * fmhip_group_sums_host is the definition on plain arrays (counts_out and every outs[i]: m floats) and needs no device. */
int fmhip_group_sums(fmhip_vec index, int64_t m, const fmhip_vec* values, int n_values /* 0 ... 4 */, uint32_t mask,
                     fmhip_vec* counts_out /* may be NULL */, fmhip_vec* outs /* n_values x popcount(mask), vector-major */,
                     int64_t* ungrouped_out /* may be NULL */);
int fmhip_group_sums_host(const float* index, int64_t n, int64_t m, const float* const* values, int n_values, uint32_t mask,
                          float* counts_out, float* const* outs, int64_t* ungrouped_out);   /* the DEFINITION; no device */

/* Tabulated functions on the device: RandomVariable.apply for a CURVE — a function tabulated on knots and interpolated: a
 * local-volatility slice, a Markov-functional numeraire, a payoff profile, an exercise boundary, an inverse empirical CDF — without the
 * vector leaving the device.  The definition is host/tabulated_function.hpp, one header for the host and the device.
 * A table: count = m knots (1 ... FMHIP_TABLE_MAX_KNOTS), finite and strictly increasing, and per function m + 1 segments of four fp64
 *   coefficients C[s][0..3].  For an element x (fp32): X = (double)x; s = the number of knots <= X (0 ... m: the last knot belongs to the
 *   right end segment); a = knots[max(s - 1, 0)], t = X - a; the result is (float)(((C3*t + C2)*t + C1)*t + C0), every operation rounded on
 *   its own in fp64, one final narrowing.  A segment with C1 = C2 = C3 = 0 yields (float)C0 for every x in it, the infinite ones included.
 *   A NaN x, and a result that is a NaN, is the quiet NaN 0x7fc00000.  At a knot that is an fp32 number the result is (float)values[i].
 * fmhip_table_build (host only): the coefficients of one function from its values at the knots, coefficients_out[(count + 1) * 4].
 *   interpolation: FMHIP_TABLE_PIECEWISE_CONSTANT (the value of the knot at or below x), FMHIP_TABLE_LINEAR, FMHIP_TABLE_CUBIC_SPLINE (natural),
 *   FMHIP_TABLE_MONOTONE_CUBIC (Fritsch-Carlson slopes: weighted harmonic mean, three-point end formula).  extrapolation: FMHIP_TABLE_CONSTANT
 *   (the end knot's value) or FMHIP_TABLE_LINEAR_EXTRAPOLATION (value and slope of the adjacent segment at the end knot).  derivative: 0, or 1
 *   for the coefficients of the derivative, (C1, 2*C2, 3*C3, 0).  With count = 1 every mode is the constant; the cubic modes need count >= 3
 *   and are the linear mode below that.
 * fmhip_table_apply: n_tables (1 ... 4, count * n_tables <= 1024) functions on the same knots, coefficients[n_tables][count + 1][4], applied
 *   to every element of x in ONE launch that reads x once: out[0 ... n_tables) are new, materialised vectors of x's size.  The device's
 *   bits EQUAL fmhip_table_apply_host's.  Elementwise: with a device list every shard runs the call on its block.
 * fmhip_table_apply_host (host only): the DEFINITION over a host float array of n (1 ... 2^31) elements, out[f][p]; needs no device.
 * Everything is checked on the host before anything is flushed or launched: counts out of range, a NULL pointer, a handle of 0, knots or
 * values that are not finite, knots that are not strictly increasing, an unknown mode -> FMHIP_ERR_INVALID_ARGUMENT;
 * FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of it is.  A build without the kernel answers
 * FMHIP_ERR_UNSUPPORTED; it never falls back. */
#define FMHIP_TABLE_MAX_KNOTS            1024
#define FMHIP_TABLE_PIECEWISE_CONSTANT   0
#define FMHIP_TABLE_LINEAR               1
#define FMHIP_TABLE_CUBIC_SPLINE         2
#define FMHIP_TABLE_MONOTONE_CUBIC       3
#define FMHIP_TABLE_CONSTANT             0   /* extrapolation: the end knot's value                          */
#define FMHIP_TABLE_LINEAR_EXTRAPOLATION 1   /* extrapolation: value and slope of the adjacent segment there */
int fmhip_table_build(const double* knots, const double* values, int count, int interpolation, int extrapolation, int derivative,
                      double* coefficients_out /* (count+1)*4 */);
int fmhip_table_apply(fmhip_vec x, const double* knots, int count, const double* coefficients /* n_tables*(count+1)*4 */, int n_tables,
                      fmhip_vec* out /* n_tables new, materialised vectors */);
int fmhip_table_apply_host(const float* x, int64_t n, const double* knots, int count, const double* coefficients, int n_tables,
                           float* const* out);

/* Named functions and option formulas per path on the device: the most common arguments of RandomVariable.apply — the
 * normal distribution function, its density, its quantile — and the closed-form prices built on them, without the vectors leaving the
 * device.  The definition is host/normal_functions.hpp, one header for the host and the device: fp64, + - * /, sqrt and the exp and log of
 * host/gamma_icdf.hpp, every operation rounded on its own; the device's bits EQUAL the host entry points'.
 * A function of an element x (fp32): X = (double)x, the result (float)f(X); a result that is a NaN is the quiet NaN 0x7fc00000.
 *   FMHIP_FN_NORMAL_DENSITY   exp(-X*X/2)/sqrt(2 pi); 0 at +-inf.
 *   FMHIP_FN_NORMAL_CDF       Phi(X); for X <= 0 the density times a piecewise fit of the Mills ratio (tools/normal_cdf_coefficients.py),
 *                             1 - Phi(-X) above; 0 at -inf, 1 at +inf.  The fp64 value is within 2^-40 relative of Phi over every fp32 x in
 *                             [-14.3, 8.3] (and the density's over [-14.3, 14.3]): the fp32 result is at most one ulp from the correctly
 *                             rounded one.
 *   FMHIP_FN_NORMAL_QUANTILE  Wichura's AS 241 in fp64; 0 -> -inf, 1 -> +inf, x < 0, x > 1 or a NaN -> NaN.
 * fmhip_function_apply: n_functions (1 ... 4) of them, kinds[f], applied to every element of x in ONE launch that reads x once:
 *   out[0 ... n_functions) are new, materialised vectors of x's size ([Phi, density] is the pair a derivative needs).
 * An option formula: a call in forward form.  Operands: forward F, volatility sigma, payoff unit N (a discount factor, a notional) — each
 *   a vector, (double) of its fp32 elements, or with a handle of 0 the fp64 scalar beside it — and the fp64 scalars maturity T >= 0 and
 *   strike K.  With s = sigma*sqrt(T):
 *   FMHIP_FORMULA_BLACK_SCHOLES  d+ = (log(F/K) + s*s/2)/s, d- = d+ - s: value N*(F*Phi(d+) - K*Phi(d-)), delta N*Phi(d+),
 *                                vega N*F*density(d+)*sqrt(T).
 *   FMHIP_FORMULA_BACHELIER      d = (F - K)/s: value N*((F - K)*Phi(d) + s*density(d)), delta N*Phi(d), vega N*sqrt(T)*density(d).
 *   An element with s <= 0, and for Black-Scholes also with F <= 0 or K <= 0, is the limit: value N*max(F - K, 0), delta N*[F > K],
 *   vega 0.  A NaN among F, sigma, N gives the quiet NaN 0x7fc00000 in every output.  A put is call - N*(F - K): the mirrors' business.
 * fmhip_option_formula: outputs is a mask of FMHIP_FORMULA_VALUE, _DELTA, _VEGA; out receives one new, materialised vector per set bit, in
 *   bit order, from ONE launch.  At least one operand is a vector, and all vectors have one size.
 * fmhip_function_apply_host, fmhip_option_formula_host (host only): the DEFINITIONS over host float arrays of n (1 ... 2^31) elements;
 *   out[f][p]; an operand array that is NULL is the scalar beside it; they need no device.
 * Both passes are elementwise: with a device list every shard runs the call on its block.  Everything is checked on the host before anything
 * is flushed or launched: counts out of range, an unknown function or model, a mask outside 1 ... 7, a NULL pointer, x = 0, no vector operand,
 * a maturity that is negative or not finite, a strike that is not finite -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes ->
 * FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of it is.  A build without
 * the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back. */
#define FMHIP_FN_NORMAL_CDF 0
#define FMHIP_FN_NORMAL_DENSITY 1
#define FMHIP_FN_NORMAL_QUANTILE 2
#define FMHIP_FORMULA_BLACK_SCHOLES 0
#define FMHIP_FORMULA_BACHELIER 1
#define FMHIP_FORMULA_VALUE 1
#define FMHIP_FORMULA_DELTA 2
#define FMHIP_FORMULA_VEGA  4
int fmhip_function_apply(fmhip_vec x, const int* kinds, int n_functions /* 1 ... 4 */, fmhip_vec* out);
int fmhip_function_apply_host(const float* x, int64_t n, const int* kinds, int n_functions, float* const* out);
int fmhip_option_formula(int model, fmhip_vec forward, double forward_scalar, fmhip_vec volatility, double volatility_scalar,
                         fmhip_vec payoff_unit, double payoff_unit_scalar, double maturity, double strike,
                         int outputs /* mask */, fmhip_vec* out /* one new vector per set bit, in bit order */);
int fmhip_option_formula_host(int model, const float* forward, double forward_scalar, const float* volatility, double volatility_scalar,
                              const float* payoff_unit, double payoff_unit_scalar, int64_t n, double maturity, double strike,
                              int outputs, float* const* out);

/* Implied volatility per path on the device: the inverse of fmhip_option_formula's value in sigma, without the vectors
 * leaving the device.  The definition is host/implied_volatility.hpp, one header for the host and the device under the rules of
 * host/normal_functions.hpp; the device's bits EQUAL the host entry point's.  A CALL in forward form; the models are FMHIP_FORMULA_*.
 * Operands: price P, forward F, payoff unit N — each a vector, (double) of its fp32 elements, or with a handle of 0 the fp64 scalar beside
 * it — and the fp64 scalars maturity T >= 0 and strike K.  Per element, in fp64: c = P/N, intrinsic = max(F - K, 0), tv = c - intrinsic,
 * decided in this order:
 *   a NaN among P, F, N; N <= 0                                        the quiet NaN 0x7fc00000 in every output
 *   c == intrinsic                                                     sigma = +0, both partials NaN
 *   T == 0; F or K infinite; c < intrinsic                             NaN in every output
 *   Black-Scholes: F <= 0 or K <= 0; c > F                             NaN in every output
 *   Black-Scholes: c == F;  Bachelier: c == +inf                       sigma = +inf, both partials NaN
 *   live: Black-Scholes intrinsic < c < F, Bachelier intrinsic < c < inf
 *                                                                      sigma the root; d_price = 1/(N*vega1), d_forward = -delta1/vega1,
 *                                                                      where vega1 and delta1 are fmhip_option_formula's with payoff unit 1
 *                                                                      at the fp64 root.  Results are narrowed to fp32 once.
 *   The fp64 root is within 1*2^-50*(|F| + |K|)/vega1 (Black-Scholes) resp. 4*2^-50*(|F| + |K|)/vega1 (Bachelier) of the exact one over
 *   the grid of DESIGN.md 4.25 (four times what was measured), and every iteration of the solver is bounded by FM_IMPLIED_MAX_ITERATIONS
 *   (64) whatever the data: an element that has not met the stopping rule by then returns its last iterate.
 * fmhip_implied_volatility: outputs is a mask of FMHIP_IMPLIED_VOLATILITY, _D_PRICE, _D_FORWARD; out receives one new, materialised vector
 *   per set bit, in bit order, from ONE launch.  At least one operand is a vector, and all vectors have one size.
 * fmhip_implied_volatility_host (host only): the DEFINITION over host float arrays of n (1 ... 2^31) elements; out[f][p]; an operand array
 *   that is NULL is the scalar beside it; it needs no device.
 * The pass is elementwise: with a device list every shard runs the call on its block.  Everything is checked on the host before anything is
 * flushed or launched: an unknown model, a mask outside 1 ... 7, a NULL pointer, no vector operand, a maturity that is negative or not
 * finite, a strike that is not finite -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH;
 * FMHIP_ERR_INVALID_HANDLE.  A refusal leaves out untouched and no vector behind.  A vector whose values were given up is the error a read
 * of it is.  A build without the kernel answers FMHIP_ERR_UNSUPPORTED; it never falls back. */
#define FMHIP_IMPLIED_VOLATILITY 1
#define FMHIP_IMPLIED_D_PRICE    2
#define FMHIP_IMPLIED_D_FORWARD  4
int fmhip_implied_volatility(int model, fmhip_vec price, double price_scalar, fmhip_vec forward, double forward_scalar,
                             fmhip_vec payoff_unit, double payoff_unit_scalar, double maturity, double strike,
                             int outputs /* mask 1 ... 7 */, fmhip_vec* out /* one new vector per set bit, in bit order */);
int fmhip_implied_volatility_host(int model, const float* price, double price_scalar, const float* forward, double forward_scalar,
                                  const float* payoff_unit, double payoff_unit_scalar, int64_t n, double maturity, double strike,
                                  int outputs, float* const* out);

/* Transform option values per path on the device: the value of a CALL in forward form under a model whose characteristic
 * function is exponential-affine in at most two state variables (Black-Scholes, Merton: none; Heston, Bates: the variance; double Heston:
 * two), given the state of every path, without the vectors leaving the device.  In Lewis' single-integral form with a fixed quadrature the
 * price is a finite sum over NODES; the node table is computed by the caller once (transform.py does it for the four named models) and is
 * data to this pass.  The definition is host/transform_formula.hpp, one header for the host and the device under the rules of
 * host/normal_functions.hpp, with the sine and cosine of host/trig64.hpp; the device's bits EQUAL the host entry point's.
 * nodes: n_nodes (1 ... FMHIP_TRANSFORM_MAX_NODES) rows of 3 + 2*n_states doubles (n_states 0 ... FMHIP_TRANSFORM_MAX_STATES):
 *   u_j, a_re, a_im, b_re[0..S), b_im[0..S), every entry finite.
 * Operands: forward F, payoff unit N and the states V_0 ... V_{S-1} - each a vector, (double) of its fp32 elements, or with a handle of 0
 * the fp64 scalar beside it (states[s], state_scalars[s]) - and the fp64 scalar strike K.  Per element, in fp64, every operation on its own:
 *   a NaN among F, N, V_s, K                   the quiet NaN 0x7fc00000 in every output
 *   not (F > 0 and K > 0)                      the limit of fmhip_option_formula: value N*max(F - K, 0), delta N*[F > K], state delta 0
 *   otherwise  k = log(F/K), and for j = 0 ... J-1 in this order
 *       e = a_re + sum_s b_re[s]*V_s,  theta = a_im + sum_s b_im[s]*V_s + u_j*k,  E = exp(e),  (s, c) = sincos(theta)
 *       G += E*c,  H -= (E*u_j)*s,  GV += E*(b_re[0]*c - b_im[0]*s)
 *     root = sqrt(F*K);  value N*(F - root*G);  delta (d/dF) N*(1 - (root/F)*(0.5*G + H));  state delta (d/dV_0, S >= 1) N*(0 - root*GV)
 *   Results are narrowed to fp32 once.  NOTHING IS CLAMPED: the value is not forced into the arbitrage bounds, and an e that overflows or a
 *   theta beyond 2^20 in size gives what IEEE 754 and the definition's sine give, a NaN (back as the quiet NaN) or an infinity.
 * fmhip_transform_option: outputs is a mask of FMHIP_TRANSFORM_VALUE, _DELTA, _STATE_DELTA; out receives one new, materialised vector per
 *   set bit, in bit order, from ONE launch.  At least one operand is a vector, and all vectors have one size.
 * fmhip_transform_option_host (host only): the DEFINITION over host float arrays of n (1 ... 2^31) elements; out[f][p]; an operand array
 *   that is NULL is the scalar beside it; it needs no device.
 * The pass is elementwise: with a device list every shard runs the call on its block.  Everything is checked on the host before anything is
 * flushed or launched: n_nodes or n_states out of range, a mask outside 1 ... 7, the state delta without a state, a NULL pointer, a table
 * entry that is not finite, no vector operand, a strike that is a NaN -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes ->
 * FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A refusal leaves out untouched and no vector behind.  A vector whose values were
 * given up is the error a read of it is.  A build without the kernel answers FMHIP_ERR_UNSUPPORTED; it never falls back. */
#define FMHIP_TRANSFORM_VALUE       1
#define FMHIP_TRANSFORM_DELTA       2
#define FMHIP_TRANSFORM_STATE_DELTA 4
#define FMHIP_TRANSFORM_MAX_NODES   256
#define FMHIP_TRANSFORM_MAX_STATES  2
int fmhip_transform_option(const double* nodes, int n_nodes, int n_states, fmhip_vec forward, double forward_scalar,
                           const fmhip_vec* states, const double* state_scalars, fmhip_vec payoff_unit, double payoff_unit_scalar,
                           double strike, int outputs /* mask 1 ... 7 */, fmhip_vec* out /* one new vector per set bit, in bit order */);
int fmhip_transform_option_host(const double* nodes, int n_nodes, int n_states, const float* forward, double forward_scalar,
                                const float* const* states, const double* state_scalars, const float* payoff_unit,
                                double payoff_unit_scalar, int64_t n, double strike, int outputs, float* const* out);

/* Nested simulation on the device: the two operations that change the SHAPE of a sample — k inner paths started from each
 * of m outer states (fmhip_vec_repeat), and the m*k inner payoffs reduced to m conditional means with their inner variances
 * (fmhip_block_moments) — without the vectors leaving the device.  The definition is host/block_moments.hpp, one header for the host and
 * the device: fp64, + - * / and comparisons.
 * A vector of n = m*block elements is m consecutive blocks of `block` elements.  For block q, S1[q] is the fp64 sum of (double)v[q*block + i]
 *   and S2[q] the fp64 sum of the exact squares (double)x*(double)x, both in ONE association that is a function of `block` alone (not of q,
 *   m, the vectors of the call, a vector's slot, the mask or the launch): segments of 2048 consecutive elements, each summed as 64 leaves —
 *   leaf l is the running sum of the segment's elements l, l + 64, ... — joined by a butterfly over the leaf index, bit 5 first; the segment
 *   sums of a block above 2048 elements are summed as one more such unit.  |S - exact| <= (fm_block_chain(block) + 1) * 2^-53 * sum|terms|.
 *   The device's outputs EQUAL fmhip_block_moments_host's bit for bit.
 * Outputs per block, each rounded to fp32 once from fp64 (a NaN result is the quiet NaN 0x7fc00000):
 *   FMHIP_BLOCK_SUM (float)S1;  FMHIP_BLOCK_MEAN (float)(S1/block);  FMHIP_BLOCK_VARIANCE (float)max(0, S2/block - (S1/block)^2), the
 *   population variance from RAW moments: absolute error about fm_block_chain(block) * 2^-53 * S2/block — adequate for the standard error
 *   of an inner estimate, no replacement for the shifted pass of fmhip_reduce_moments.  NaN and +-inf propagate as fp64 arithmetic
 *   propagates them, inside their block only.
 * fmhip_block_moments: n_vs = 1 ... 4 vectors of one size n (1 ... 2^31 - 1, a multiple of block >= 1), each read once; mask: at least one
 *   of the three bits; outs[i*popcount(mask) + j] = a new, materialised vector of n/block elements, j over the set bits in ascending order.
 * fmhip_block_moments_host: the DEFINITION over a host float array: outs[j*(n/block) + q]; needs no device.
 * fmhip_vec_repeat: *out = a new, materialised vector of n*each*times (<= 2^31 - 1) elements, out[(t*n + p)*each + e] = v[p] copied bit
 *   for bit (a NaN keeps its payload, a zero its sign): each = k, times = 1 starts k inner paths per outer state; each = 1 tiles.
 * Everything is checked on the host before anything is flushed or launched: n_vs outside 1 ... 4, a mask of 0 or with unknown bits,
 * block < 1, n no multiple of block, each < 1, times < 1, an output beyond 2^31 - 1 elements, a NULL pointer, a handle of 0 ->
 * FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were
 * given up is the error a read of it is.  A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.  With a device
 * list of more than one shard both device calls answer FMHIP_ERR_UNSUPPORTED (blocks would straddle the shards); under an expectation
 * communicator they act on this rank's own vector, as fmhip_vec_read_elements does. */
#define FMHIP_BLOCK_SUM 1u
#define FMHIP_BLOCK_MEAN 2u
#define FMHIP_BLOCK_VARIANCE 4u
int fmhip_block_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, fmhip_vec* outs);
    /* outs[i*popcount(mask) + j]: new vectors of size n/block, j in ascending bit order */
int fmhip_block_moments_host(const float* v, int64_t n, int64_t block, uint32_t mask, float* outs);   /* the DEFINITION; no device */
int fmhip_vec_repeat(fmhip_vec v, int64_t each, int64_t times, fmhip_vec* out);

/* Block order statistics on the device: what a nested risk measure needs of the m*k inner values beside their moments — the
 * quantile of every block (dynamic initial margin, nested VaR), the mean of a tail of it (expected shortfall), its minimum and maximum,
 * bootstrap percentile intervals per block — and the blocks sorted, without the vectors leaving the device.  The definition is
 * host/block_order.hpp, one header for the host and the device.
 * A vector of n = m*block elements is m consecutive blocks of `block` elements, 1 <= block <= 4096 (FM_BLOCK_ORDER_MAX).  s_q is block q in
 *   ascending order of the 32-bit key of fmhip_select_ranks_batch — the order of java.util.Arrays.sort(float[]): -0.0 before +0.0, every NaN
 *   equal and last.  Equal keys have equal bits apart from NaNs, so everything below is a function of the block's multiset alone (not of q,
 *   m, the vectors of the call, a vector's slot, the other selectors or the launch).
 *   The device's outputs EQUAL the _host calls' bit for bit.
 * Rank r (0 <= r < block): out[q] = s_q[r], an element of the block bit for bit (the sign of a zero, a denormal); a position in the NaN tail
 *   gives the quiet NaN 0x7fc00000.  Duplicate ranks are allowed.
 * Range mean [from, to] (0 <= from <= to < block): S = the fp64 sum of s_q[from..to] in the association fmhip_block_moments gives a block of
 *   to - from + 1 elements (64 strided leaves from -0.0 per 2048 terms, the butterfly with bit 5 first, one more unit above 2048 terms);
 *   out[q] = (float)(S / (to - from + 1)), rounded once.  A range that reaches the NaN tail, or that holds both infinities, gives 0x7fc00000.
 * fmhip_block_order_statistics: n_vs = 1 ... 4 vectors of one size n (1 ... 2^31 - 1, a multiple of block), each read once; n_ranks = 0 ... 8,
 *   n_ranges = 0 ... 4, at least one selector; outs[i*(n_ranks + n_ranges) + j] = a new, materialised vector of n/block elements, ranks first.
 * fmhip_block_sort: *out = a new, materialised vector of n elements, out[q*block + i] = s_q[i]; every NaN comes back as 0x7fc00000.  Keys are
 *   carried, not (key, index) pairs: fmhip_sort_by_key is the stable, payload-preserving sort.
 * The _host calls are the DEFINITION over a host float array (outs[j*(n/block) + q]); they need no device.
 * Everything is checked on the host before anything is flushed or launched: n_ranks + n_ranges == 0, a count outside its limits, a rank or a
 * range outside the block, from > to, block < 1, n no multiple of block, a NULL pointer, a handle of 0 -> FMHIP_ERR_INVALID_ARGUMENT;
 * block > 4096 -> FMHIP_ERR_UNSUPPORTED (fmhip_select_ranks_batch selects in whole vectors, fmhip_sort_by_key sorts them); vectors of
 * different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of it is.
 * A build without the kernel answers FMHIP_ERR_UNSUPPORTED; it never falls back.  With a device list of more than one shard both device
 * calls answer FMHIP_ERR_UNSUPPORTED (blocks would straddle the shards); under an expectation communicator they act on this rank's own
 * vector, as fmhip_block_moments does. */
int fmhip_block_order_statistics(const fmhip_vec* vs, int n_vs, int64_t block, const int64_t* ranks, int n_ranks,
                                 const int64_t* range_from, const int64_t* range_to, int n_ranges, fmhip_vec* outs);
    /* outs[i*(n_ranks+n_ranges) + j]: new vectors of size n/block, ranks first */
int fmhip_block_order_statistics_host(const float* v, int64_t n, int64_t block, const int64_t* ranks, int n_ranks,
                                      const int64_t* range_from, const int64_t* range_to, int n_ranges, float* outs);   /* the DEFINITION; no device */
int fmhip_block_sort(fmhip_vec v, int64_t block, fmhip_vec* out);
int fmhip_block_sort_host(const float* v, int64_t n, int64_t block, float* out);                                        /* the DEFINITION; no device */

/* Order statistics ACROSS vectors, per path: the largest, second largest, r-th largest of K assets on every path and WHICH
 * asset it is — best-of, worst-of, rainbow and mountain-range payoffs, the r-th default of a basket, the ordered-price regression basis of a
 * Bermudan max-call — from one launch, without the vectors leaving the device.  The definition is host/cross_order.hpp, one header for the
 * host and the device.
 * K = n_vs = 1 ... 32 vectors of one size n (1 ... 2^31 - 1); the same handle may stand in several slots.  For path p the K pairs
 *   (key of vs[i][p], i) are sorted ascending by the 32-bit key of fmhip_select_ranks_batch — the order of java.util.Arrays.sort(float[]):
 *   -0.0 before +0.0, every NaN equal and last — ties by slot i: a stable sort.
 *   The device's outputs EQUAL the _host calls' bit for bit.
 * Value of rank r (0 <= r < K): out[p] = the r-th smallest of the path's K values, one of them bit for bit; a position in the NaN tail gives
 *   the quiet NaN 0x7fc00000.  Index of rank r: out[p] = the slot i of that pair as a float (exact: at most 31).
 * fmhip_cross_order_statistics: n_ranks = 1 ... 32 selectors, duplicates allowed; outputs is a mask of FMHIP_CROSS_VALUES and
 *   FMHIP_CROSS_INDICES.  outs receives new, materialised vectors of n elements: the values of all selectors (if asked for), then the indices.
 *   An output depends on the path's K values and on r alone: not on n, the other selectors, the mask, the launch, or where the path sits.
 * fmhip_cross_select: *out = a new, materialised vector, out[p] = vs[j][p] bit for bit where index[p] is an integer j in [0, K), and the quiet
 *   NaN 0x7fc00000 for every other index[p] (a fraction, a negative, a value >= K, a NaN, an infinity): what carries a payload behind an index
 *   output.  The index is range-checked before it picks a vector: no index faults.
 * The _host calls are the DEFINITION over host float arrays (vs[i], outs[o]: n floats each); they need no device.
 * Everything is checked on the host before anything is flushed or launched: a count outside its limits, a rank outside [0, K), a mask
 * outside 1 ... 3, a NULL pointer, a handle of 0 -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes -> FMHIP_ERR_SIZE_MISMATCH;
 * FMHIP_ERR_INVALID_HANDLE.  A refusal leaves outs untouched and no vector behind.  A build without the kernel answers
 * FMHIP_ERR_UNSUPPORTED; it never falls back.  Elementwise: per shard with a device list, local to the rank under a communicator. */
#define FMHIP_CROSS_VALUES 1
#define FMHIP_CROSS_INDICES 2
int fmhip_cross_order_statistics(const fmhip_vec* vs, int n_vs, const int* ranks, int n_ranks, int outputs, fmhip_vec* outs);
    /* outs[j], then outs[n_ranks + j] with both bits: new vectors of size n */
int fmhip_cross_order_statistics_host(const float* const* vs, int n_vs, int64_t n, const int* ranks, int n_ranks, int outputs,
                                      float* const* outs);                                                /* the DEFINITION; no device */
int fmhip_cross_select(fmhip_vec index, const fmhip_vec* vs, int n_vs, fmhip_vec* out);
int fmhip_cross_select_host(const float* index, const float* const* vs, int n_vs, int64_t n, float* out);  /* the DEFINITION; no device */

/* Kernel regression on the device: kernel-weighted LOCAL MOMENTS of up to four vectors at a grid of points of a key vector
 * in one pass — E[y | x = p_q] as a curve: the inner step of the particle method for local-stochastic-volatility calibration
 * (E[v_t | S_t = S] at every time step), kernel density estimates, smooth exercise boundaries, exposure profiles — without the vectors
 * leaving the device.  The definition is host/kernel_regression.hpp, one header for the host and the device.
 * points[n_points]: finite, non-decreasing doubles, 1 <= n_points <= FMHIP_KERNEL_MAX_POINTS; bandwidths[n_points]: finite, > 0.  Per point,
 *   one fp64 rounding each: lower_q = p_q - h_q, upper_q = p_q + h_q, rh_q = 1.0 / h_q.  BOTH lower and upper must be non-decreasing in q (one
 *   bandwidth for all points always is; bandwidths that widen in the tails are when they widen slowly enough).
 * Membership: with xd = (double)key[i], element i is a member of point q iff lower_q < xd && xd < upper_q.  A NaN or infinite key is a
 *   member of no point.
 * Weight of a member, in fp64, every operation rounded on its own: d = xd - p_q; u = d*rh_q; t = 1 - u*u; w = 1 (FMHIP_KERNEL_UNIFORM),
 *   1 - |u| (TRIANGULAR), t (EPANECHNIKOV), t*t (QUARTIC), (t*t)*t (TRIWEIGHT); then w = w < 0 ? 0 : w.  No Gaussian: its support is not
 *   compact.
 * sums_out[n_points][entries], the fp64 SUMS over the members, yd_m = (double)y_m[i], n_y = 0 ... 4:
 *   order 0: [w, w*yd_0, ...]                                         entries = 1 + n_y
 *   order 1: [w, e1 = w*d, e1*d, w*yd_0, ..., e1*yd_0, ...]           entries = 3 + 2*n_y
 *   Normalisation constants (3/4, 1/(n*h)) are the caller's.  No float atomics.  The bits of one (point, entry) sum are a function of n, of
 *   which path positions are members and of the values there — not of the other points, n_y, or the position of a vector in y; w, w*d and
 *   w*d*d are the same bits for both orders.  ONE launch.
 * fmhip_kernel_moments_host: the DEFINITION over host float arrays; needs no device; a point's members are added in path order.  The
 *   device's sums agree with any summation order's to 2*members*2^-53*sum|terms| per (point, entry).
 * Everything is checked on the host before anything is flushed or launched, by one function for the device and the host entry point:
 * counts out of range, an unknown kernel or order, a NULL pointer, points or bandwidths that are not finite, a bandwidth <= 0, points, lower
 * or upper that decrease, a 0 among y or as the key, n == 0 -> FMHIP_ERR_INVALID_ARGUMENT; vectors of different sizes ->
 * FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of it is.  A build without the
 * kernel answers FMHIP_ERR_UNSUPPORTED; it never falls back.  With a device list the sums add in shard order; with an expectation
 * communicator they are those of the GLOBAL sample (one gather, added in rank order). */
#define FMHIP_KERNEL_MAX_POINTS   256
#define FMHIP_KERNEL_UNIFORM      0
#define FMHIP_KERNEL_TRIANGULAR   1
#define FMHIP_KERNEL_EPANECHNIKOV 2
#define FMHIP_KERNEL_QUARTIC      3
#define FMHIP_KERNEL_TRIWEIGHT    4
int fmhip_kernel_moments(fmhip_vec key, const double* points, const double* bandwidths, int n_points, int kernel, int order,
                         const fmhip_vec* y, int n_y, double* sums_out);
int fmhip_kernel_moments_host(const float* key, int64_t n, const double* points, const double* bandwidths, int n_points, int kernel, int order,
                              const float* const* y, int n_y, double* sums_out);

/* Polynomial regression in one pass: the normal equations of a regression on a POLYNOMIAL basis — the Longstaff-Schwartz
 * basis of a product on several underlyings — from the state vectors alone, and the fitted polynomial as a new vector.  The monomials are
 * never in memory: the moments kernel forms them in registers as the operands of fmhip_cross_moments_wide's pass.
 * states: n_states vectors (1 ... 8), all of one size n > 0.  exponents[n_terms][n_states], each entry 0 ... 6: term i is the monomial
 *   prod_s states[s]^exponents[i*n_states + s].  extra_x: n_extra >= 0 ordinary vectors among the regressors (an exercise value, a spline); a
 *   handle of 0 there is the constant 1, as in the wide call.  y: n_y >= 0 dependents.  n_terms >= 1; n_terms + n_extra + n_y <= 64 for the
 *   moments, n_terms + n_extra <= 60 for the evaluation.  The regressor list is: the terms in the order given, then extra_x (then y).
 * How a term is computed — the contract: u^e is u followed by e - 1 multiplications by u, each rounded to fp32: ((u*u)*u)...; the term is
 *   the product of the powers with e > 0 in ascending state index, left to right, each product rounded to fp32, nothing contracted.  A state
 *   with exponent 0 does not take part (it is not multiplied by 1, so inf^0 is no NaN).  The all-zero tuple is the constant 1.0f: it is not
 *   loaded and behaves as a handle of 0 does in fmhip_cross_moments.
 * fmhip_polynomial_cross_moments: sums_out has exactly the layout of fmhip_cross_moments with n_x = n_terms + n_extra.  The sums are, bit
 *   for bit, those fmhip_cross_moments_wide returns for the same list with the terms materialised by the chain above: the same tree (chunks
 *   of 64 paths, the waves in order, the workgroups in order; its bits depend on n and the pair's values only).  ONE launch.
 * fmhip_polynomial_evaluate: *out = a new, materialised vector r = ((t_0*c_0) + t_1*c_1) + ... over the terms, then the extra vectors, with
 *   c_i = (float)coefficients[i]: every product and every sum rounded to fp32 — what basis[0].mult(c0).addProduct(basis[1], c1)... computes on
 *   the materialised basis.  Eager: pending operands are computed in one flush, one launch follows.
 * The _host functions are the DEFINITION over host float arrays (a NULL among extra_x is the constant 1) and need no device; they add in
 *   path order.  The device's sums agree with them to (xmom_wide_chain(n) + 1)*2^-53*sum|a*b| per entry (csrc/xmom_wide_kernel.h).
 * Everything is checked on the host before anything is flushed or launched, by one function for the device and the host entry point:
 * counts out of range, an exponent above 6, a NULL pointer, a 0 among states or y, n == 0 -> FMHIP_ERR_INVALID_ARGUMENT; vectors of
 * different sizes -> FMHIP_ERR_SIZE_MISMATCH; FMHIP_ERR_INVALID_HANDLE.  A vector whose values were given up is the error a read of it is.
 * A build without the kernels answers FMHIP_ERR_UNSUPPORTED; it never falls back.  With a device list the sums add in shard order and the
 * evaluation is per shard; with an expectation communicator the sums are those of the GLOBAL sample (one gather, added in rank order). */
int fmhip_polynomial_cross_moments(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms,
                                   const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, double* sums_out);
int fmhip_polynomial_evaluate(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms,
                              const fmhip_vec* extra_x, int n_extra, const double* coefficients, fmhip_vec* out);
int fmhip_polynomial_cross_moments_host(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms,
                                        const float* const* extra_x, int n_extra, const float* const* y, int n_y, double* sums_out);
int fmhip_polynomial_evaluate_host(const float* const* states, int64_t n, int n_states, const uint8_t* exponents, int n_terms,
                                   const float* const* extra_x, int n_extra, const double* coefficients, float* out);

/* Expectation communicator: Monte-Carlo paths sharded over processes (one GPU each) behind an UNCHANGED caller.
 * Every vector of this process holds the paths [rank·n, (rank+1)·n) of a global vector of world·n paths; all element-wise
 * work is local; the one thing that couples paths is an expectation.  With a communicator set, fmhip_reduce_moments and
 * fmhip_reduce_moments_batch return the moments of the GLOBAL vector on every rank: the local {Σ, Σ², min, max} are handed to
 * `gather` (called on the host, by the thread that asked; it must deliver every rank's `count` doubles to every rank, in rank
 * order — an all-gather over RCCL / MPI / gloo) and combined by fmhip_expectation_combine: sums added in RANK ORDER (bitwise
 * equal on every rank, whatever the transport), min / max over ranks.  The drop-in classes divide by world·n
 * (fmhip_expectation_world), so getAverage() / getVariance() of a finmath-lib product mean the same as on one GPU and every
 * rank's optimiser takes the same step.  The *_device variants stay local partials (for callers that run their own collective
 * on the device).  Every rank must ask for the same expectations in the same order.  world = 1 or gather = NULL removes it.
 * The order statistics above are those of the GLOBAL sample too (their per-pass counts go through `gather` as doubles, exact below 2^53):
 * every rank asks for the same ranks / bounds in the same order, like expectations.  So are the cross moments (their sums go through `gather` once).
 * The reference has nothing here: one process, one device (RandomVariableCuda.java:161,177). */
typedef int (*fmhip_gather_fn)(void* context, const double* local, int count_doubles, double* gathered /* [world][count_doubles] */);
int fmhip_set_expectation_comm(int world, int rank, fmhip_gather_fn gather, void* context);
/* The communicator's size and this process's rank (1 and 0 without one). */
int fmhip_expectation_world(int* world, int* rank);
/* The combination rule on its own (host only, needs no device): gathered[r·count + k] = rank r's moments of vector k. */
int fmhip_expectation_combine(const fmhip_moments* gathered, int world, int count, fmhip_moments* out);

/* ---------------------------------------------------------------- fused programs */

/* One SSA instruction. Values are numbered: 0 … n_inputs-1 are the program inputs, n_inputs+i is the
 * result of ops[i]. Unused operands are -1. */
typedef struct fmhip_prog_op {
    int32_t opcode;     /* fmhip_opcode */
    int32_t a, b, c;    /* operand value ids */
    double  scalar;     /* narrowed to float, used by the *_S / v2s1 opcodes */
} fmhip_prog_op;

/* Compile an op stream once. out_values[n_outputs]: value ids materialised as new vectors;
 * reduce_values[n_reduce] (n_reduce <= 2): value ids reduced to fmhip_moments inside the same launch. */
int fmhip_program_create(const fmhip_prog_op* ops, int n_ops, int n_inputs,
                         const int32_t* out_values, int n_outputs,
                         const int32_t* reduce_values, int n_reduce,
                         fmhip_program* out);
int fmhip_program_release(fmhip_program p);
/* Number of kernel launches one run of p takes (1 unless the program had to be split). */
int fmhip_program_launch_count(fmhip_program p, int* n_launches);
/* Inputs, outputs and fused reductions per batch row of p: the lengths fmhip_program_run expects of its arrays. */
int fmhip_program_shape(fmhip_program p, int* n_inputs, int* n_outputs, int* n_reduce);
/* Run p over `batch` independent input tuples in ONE launch (horizontal batching).
 *   inputs  [batch * n_inputs ]  all of equal size
 *   outputs [batch * n_outputs]  receives new handles (caller releases)
 *   reduce_shift [n_reduce] or NULL (=0)
 *   moments [batch * n_reduce] host results, or NULL to skip the host read-back
 *   device_moments: optional device buffer of batch*n_reduce*4 doubles, or NULL */
int fmhip_program_run(fmhip_program p, int batch,
                      const fmhip_vec* inputs, fmhip_vec* outputs,
                      const double* reduce_shift, fmhip_moments* moments, void* device_moments);
/* As fmhip_program_run, but writes into caller-provided existing output vectors (no allocation);
 * an output may alias an input of the same row. */
int fmhip_program_run_into(fmhip_program p, int batch,
                           const fmhip_vec* inputs, const fmhip_vec* outputs,
                           const double* reduce_shift, fmhip_moments* moments, void* device_moments);

/* ---------------------------------------------------------------- execution tiers
 * A compiled program (explicit, or built by the lazy front-end) starts on the bytecode interpreter kernel and may be
 * promoted to a SPECIALISED kernel: straight-line gfx950 code generated from its op stream and compiled at run time
 * (hiprtc) on a background thread.  Both tiers are built from the same device functions with the same floating-point
 * flags and give bit-identical results.  The reference has no counterpart (one precompiled PTX kernel per method,
 * RandomVariableCuda.java:78-117, :539-557). */
#define FMHIP_JIT_OFF  0     /* interpreter only */
#define FMHIP_JIT_AUTO 1     /* default: explicit programs at creation, lazy programs once they are hot; asynchronous */
#define FMHIP_JIT_SYNC 2     /* compile before the first launch (deterministic tier: tests, benchmarks) */
/* Default from the environment variable FMHIP_JIT = off | auto | sync. */
int fmhip_set_jit(int mode, int* previous);
/* Blocks until every queued compilation has finished. */
int fmhip_jit_wait(void);
/* compiled = kernels ready (of which disk_cache_hits were loaded from the persistent code-object cache,
 * $FMHIP_JIT_CACHE_DIR, default ~/.cache/fmhip-jit, "off" disables), compile_seconds = host time spent on them. */
int fmhip_jit_stats(int64_t* compiled, int64_t* failed, int64_t* pending, double* compile_seconds, int64_t* disk_cache_hits);
/* *tier: 0 = interpreter, 1 = specialised kernel ready (the next launch uses it); *vgprs = its register count. */
int fmhip_program_tier(fmhip_program program, int* tier, int* vgprs);
/* The generated source of a program's specialised kernel (needs no device).  Copies at most `capacity` bytes
 * including the terminating 0 and stores the full length (without the 0) in *needed. */
int fmhip_program_source(const fmhip_prog_op* ops, int n_ops, int n_inputs, const int32_t* out_values, int n_outputs,
                         const int32_t* reduce_values, int n_reduce, char* buffer, int64_t capacity, int64_t* needed);

/* ---------------------------------------------------------------- Brownian increments */

/* Fill n_steps*n_factors new vectors of n_paths N(0, dt_step) increments:
 *   out[step*n_factors + factor][p] = (float)sqrt(dt[step]) * Z(seed, step, factor, path_offset + p)
 * Z is a counter-based normal — Philox4x32-10 (counter = (global path index / 4, step * n_factors + factor), key = seed), each 32-bit
 * word mapped through the inverse normal CDF (a segment table in LDS and a cubic per segment: csrc/fm_normal_table.hpp) — a pure
 * function of (seed, step, factor, global path index), hence independent of launch geometry and of how paths are sharded over GPUs.
 * Replaces curandGenerateNormal per (step,factor) (BrownianMotionCudaWithRandomVariableCuda.java:168-178). */
int fmhip_bm_generate(int64_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                      const double* dt, fmhip_vec* out);

/* Host-side Mersenne-Twister Brownian motion (restatement of finmath-lib's BrownianMotionFromMersenneRandomNumbers, the
 * generator the reference's tests feed to every factory: LIBORMarketModelCalibrationATMTest.java:283): MT19937 seeded like
 * commons-math3 MersenneTwister(int), nextDouble(), inverse normal CDF (AS 241), times sqrt(dt); draw order path-major.
 * fmhip_mersenne_increments fills host doubles out[(step*n_factors+factor)*n_paths + path] and needs no device;
 * fmhip_bm_generate_mersenne uploads them as n_steps*n_factors vectors (narrowed to fp32 like any double[] upload). */
int fmhip_mersenne_increments(int32_t seed, int n_steps, int n_factors, int64_t n_paths, const double* dt, double* host_out);
int fmhip_bm_generate_mersenne(int32_t seed, int n_steps, int n_factors, int64_t n_paths, const double* dt, fmhip_vec* out);
/* The same increments GENERATED ON THE DEVICE: MT19937 is linear over GF(2), so every workgroup enters the one stream at its own
 * segment by jump-ahead; no host vector, no upload.  out[k] holds paths path_offset … path_offset + n_paths of vector k of the
 * whole motion, so a shard or a rank generates its own block without drawing what precedes it (2·n_steps·n_factors·(path_offset +
 * n_paths) <= 2^44 words, an error beyond).  Contract against fmhip_mersenne_increments narrowed to fp32: the 52-bit uniforms are
 * the host's bit for bit; a draw with |u - 0.5| <= 0.425 (85 %) goes through + - * / only and is EQUAL; a tail draw goes through
 * log, where the device library and the host's libm may differ by an fp64 ulp: equal too, except that about one in 10^8 may differ
 * by one fp32 ulp.  Arguments are checked on the host before anything is flushed or launched (negative time steps are an error
 * here).  A build without the kernel returns FMHIP_ERR_UNSUPPORTED; it never falls back to the host generator. */
int fmhip_bm_generate_mersenne_device(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out);
/* Independent increments with a LAW PER (TIME STEP, FACTOR) from the same MT19937 stream: one nextDouble() u per increment, path-major
 * (path, step, factor), pushed through an inverse CDF — what finmath-lib's IndependentIncrementsFromICDF, JumpProcessIncrements and the
 * three-factor layout of MonteCarloMertonModel draw [unverified: finmath-lib is not vendored; restated from its documentation].
 * kinds, a, b: [n_steps * n_factors], index step * n_factors + factor.
 *   FMHIP_LAW_NORMAL   inverseNormalCdf(u) * a      a >= 0 (sqrt(dt) for a Brownian factor, 1 for a jump size); b ignored
 *   FMHIP_LAW_UNIFORM  a + (b - a) * u              a <= b, finite
 *   FMHIP_LAW_POISSON  min { k >= 0 : F[k] >= u }   a = the mean (lambda * dt), 0 <= a <= 128; b ignored; F is a table built on the
 *                      host in fp64, once per distinct mean: F[0] = p = exp(-a), p = p * a / k, F[k] = F[k-1] + p, last entry 1.0
 * fmhip_increments_host is the definition (doubles, layout as fmhip_mersenne_increments, no device).  With every law NORMAL and
 * a = sqrt(dt[step]) it returns fmhip_mersenne_increments' doubles bit for bit.
 * fmhip_increments_generate_device generates paths path_offset ... path_offset + n_paths of the same numbers on the device (narrowed
 * to fp32 once): Poisson and uniform draws EQUAL the definition's (the device only compares u with the host's table), normal draws
 * under the contract of fmhip_bm_generate_mersenne_device.  Both check their arguments with one function, before anything is flushed
 * or launched: an unknown kind, a NaN or negative scale or mean, a mean above 128, a > b or non-finite bounds, more than 2^24 laws, words
 * beyond 2^44, more than 2^16 table entries over all distinct means -> FMHIP_ERR_INVALID_ARGUMENT.  A build without the kernel returns
 * FMHIP_ERR_UNSUPPORTED; it never falls back to the host definition.
 * Two more laws, for pure-jump Levy processes (gamma, variance-gamma), through the same two entry points:
 *   FMHIP_LAW_GAMMA        fm_inverse_gamma_cdf(a, consts, u) * b   a = the shape, 0.01 <= a <= 1000; b = the scale, finite and > 0
 *   FMHIP_LAW_EXPONENTIAL  -fm_log64(1 - u) / a                     a = the rate, finite and > 0; b ignored
 * Their definition, host/gamma_icdf.hpp, is one header that the host and the device both compile: exp, log, the incomplete gamma function
 * and its inverse (Halley steps) written with + - * /, sqrt and integer operations only, every operation rounded once.  These draws of
 * fmhip_increments_generate_device EQUAL the definition's, every one; u = 0 gives +0.0.  consts (lgamma(shape), 1/shape, ...) is computed
 * on the host once per distinct shape and shares the 2^16 table entries with the Poisson tables.  A call that names one of these laws
 * runs fm_mt_levy_kernel, any other call the kernel it ran before.  A shape outside the range, a non-positive, NaN or infinite shape,
 * scale or rate -> FMHIP_ERR_INVALID_ARGUMENT.  Kind 3 is not a law. */
enum { FMHIP_LAW_NORMAL = 0, FMHIP_LAW_UNIFORM = 1, FMHIP_LAW_POISSON = 2 };
enum { FMHIP_LAW_GAMMA = 4, FMHIP_LAW_EXPONENTIAL = 5 };
int fmhip_increments_host(int32_t seed, int n_steps, int n_factors, int64_t n_paths,
                          const int32_t* kinds, const double* a, const double* b, double* host_out);
int fmhip_increments_generate_device(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                                     const int32_t* kinds, const double* a, const double* b, fmhip_vec* out);
/* QUASI-MONTE-CARLO: Brownian increments from a Sobol' sequence, with a Brownian bridge (what finmath-lib's SobolSequence taken through
 * BrownianMotionFromRandomNumberGenerator and BrownianBridge serve [unverified: finmath-lib is not vendored; names from its documentation]).
 * The definition is host/sobol.hpp, one header that the host and the device both compile:
 *   point        Joe & Kuo's direction numbers (new-joe-kuo-6), 1024 dimensions, 30 bits, Gray-code order, origin skipped: global path p
 *                uses index i = p + 1, x(i, d) = XOR over the set bits j of i ^ (i >> 1) of v[d][j]; i < 2^30
 *   shift        randomize = 1: shift[d] = MT19937(seed) next 32-bit word >> 2, d = 0, 1, ... (the seeding of fmhip_mersenne_increments);
 *                randomize = 0: none.  u = (x ^ shift[d]) * 2^-30 + 2^-31, exact, never 0 or 1
 *   normal       AS 241 with a portable logarithm in the tails (+ - * / sqrt only): the same bits on the host and on the device
 *   construction FMHIP_SOBOL_INCREMENTAL: dimension step * n_factors + factor, increment z * sqrt(dt[step]).
 *                FMHIP_SOBOL_BRIDGE: times t_0 = 0, t_(k+1) = t_k + dt[k]; node 0 is W(t_n) = sqrt(t_n - t_0) * z; then, breadth first from
 *                (0, n): an interval (l, r) with r - l >= 2 gets m = (l + r) / 2, W_m = a W_l + (1 - a) W_r + sd z, a = (t_r - t_m) / (t_r -
 *                t_l), sd = sqrt((t_m - t_l)(t_r - t_m) / (t_r - t_l)), and is split into (l, m), (m, r).  Node k of a factor uses
 *                dimension k * n_factors + factor; the increment of step j is W_(j+1) - W_j.  fp64, narrowed to fp32 once.
 * fmhip_sobol_points_host: u_out[k * n_dims + d] = u of index first_index + k (index 0 is the origin), no device.
 * fmhip_sobol_increments_host: the definition; host_out[(step * n_factors + factor) * n_paths + k] = increment of global path path_offset + k
 * (doubles; no device).  fmhip_bm_generate_sobol_device: the same paths generated on the device (fm_sobol_bm_kernel), every increment EQUAL
 * to the definition's narrowed to fp32; out as fmhip_bm_generate_mersenne_device's.  One function checks the arguments of both, before
 * anything is flushed or launched: n_steps * n_factors <= 1024, dt finite and > 0 (bridge) or >= 0 (incremental), a known construction,
 * randomize 0 or 1, path_offset >= 0, path_offset + n_paths < 2^30, else FMHIP_ERR_INVALID_ARGUMENT.  A build without the kernel returns
 * FMHIP_ERR_UNSUPPORTED; it never falls back to the host definition. */
enum { FMHIP_SOBOL_INCREMENTAL = 0, FMHIP_SOBOL_BRIDGE = 1 };
int fmhip_sobol_points_host(int n_dims, int64_t first_index, int64_t count, int32_t seed, int randomize, double* u_out);
int fmhip_sobol_increments_host(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                                const double* dt, double* host_out);
int fmhip_bm_generate_sobol_device(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset,
                                   const double* dt, fmhip_vec* out);
/* Inverse of the standard normal CDF (Wichura AS 241 / PPND16), exposed for tests. Returns the value (no status). */
double fmhip_inverse_normal_cdf(double p);

/* ---------------------------------------------------------------- pool */

/* Return cached (unused) device buffers to the driver (DeviceMemoryPool.clean, :393). */
int fmhip_pool_clean(void);
/* clean + drop every cached buffer; live vectors stay valid (DeviceMemoryPool.purge, :424). */
int fmhip_pool_purge(void);
int fmhip_pool_stats(fmhip_pool_stats_t* out);

/* ---------------------------------------------------------------- measurement */

/* While enabled, every launch of the fused-program kernel is bracketed by a pair of HIP events on the
 * runtime stream.  fmhip_profile_read blocks until the recorded launches have finished, returns the sum
 * of their device durations (ms) and their count, and clears the record.  Used by bench.py for the live
 * roofline figure; adds two event records per launch, so leave it off in production. */
int fmhip_profile_enable(int enabled);
/* Algorithmic bytes of all program launches so far (4 B x N x (inputs read + outputs written) per batch row;
 * reductions add nothing) and how many of those launches ran on the specialised tier. */
int fmhip_traffic_stats(int64_t* algorithmic_bytes, int64_t* specialised_launches);
/* Counters of the engine's work so far (all engines of the process added up; every field an int64, `size` = bytes filled in).
 * The reference keeps no such record; the nearest are the log lines of DeviceMemoryPool (RandomVariableCuda.java:287-296).
 *   values_deferred / _now / values_demanded: results of recorded methods that a fused launch computed for its consumers and did NOT
 *   store although the caller still held a handle (the engine has learnt that handles at such positions are never used again — a
 *   garbage-collected caller holds one for EVERY temporary until its next collection), how many of them exist now, and how many were
 *   wanted after all (computed again from their recipe and stored: each costs a launch, and teaches the engine to store that position). */
typedef struct fmhip_engine_stats_t {
    int64_t size;
    int64_t kernel_launches, specialised_launches, interpreter_launches;
    int64_t algorithmic_bytes, algorithmic_bytes_written;
    int64_t values_deferred, values_deferred_now, values_demanded;
    int64_t pending_operations;
    int64_t peak_bytes_reserved;
    /* releases that arrived from a thread which only ever releases (a collector's cleaner): queued, and performed by a driving thread
     * while it waited for the device / at once because too many waited; the time the driving threads spent on them */
    int64_t late_releases_while_waiting, late_releases_at_once, late_release_nanoseconds;
    /* launches that served several components of one loop shape reading the same sequence of vectors (each vector loaded once for all of
     * them: the swaptions of one exercise date), and how many components they served */
    int64_t merged_launches, merged_chains;
    /* rows of batched launches that were not computed because an earlier row of the same launch read the same vectors with the same
     * scalars (the parameter sets of a finite-difference batch before their bumped parameter matters): they share its vectors */
    int64_t common_rows;
    /* launches of a loop kernel: the rolled stretch of a component, its peeled form (head, loop and tail), a merged family */
    int64_t rolled_launches;
} fmhip_engine_stats_t;
int fmhip_engine_stats(fmhip_engine_stats_t* out);
int fmhip_profile_read(double* kernel_ms_total, int64_t* n_launches);

#ifdef __cplusplus
}
#endif
#endif /* FMHIP_H */
