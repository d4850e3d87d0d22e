// sharded.hpp — ONE process driving SEVERAL devices behind the unchanged C-ABI (fmhip_init_devices).
//
// The path shards by Monte-Carlo paths: every vector of n paths is cut into contiguous blocks (boundaries at multiples of four paths:
// one Philox call covers four), block d lives on device d, every element-wise method runs on every block, and only expectations
// couple the blocks.  Design: one ENGINE per device shard (the single-device engine, unchanged: its own stream, pool, row-table ring,
// arrival counters, moments arena, specialised-kernel tier), each driven by a WORKER thread of its own; the caller's C-ABI calls are
// replayed on every worker, in order, through the very same entry points (a worker thread's Engine::get() is its shard's engine).
// The caller's handles are the front's own numbers; each worker keeps the table front handle → its engine's handle.  Calls that
// return nothing but handles are posted and return at once — the front checks what can be checked without the engines (handles,
// sizes, opcode shapes), anything else a shard reports (a device allocation that fails …) surfaces at the next call that waits.  Calls
// that return data wait for all shards: a read gathers the blocks by one device-to-host copy per shard, straight into the caller's
// buffer; host-side moments need NO collective — every shard's launch leaves its 32 bytes in pinned memory, the front adds them in
// shard order by the rule fmhip_expectation_combine implements (sums in shard order, java.lang.Math.min / max).  Nothing is exchanged
// between devices for those.  Expectations wanted ON the devices (fmhip_reduce_moments_batch_devices; the *_device variants deliver to
// the first listed device) are the one exchange: a grouped RCCL all-gather of the shards' moments over the listed devices and a combine
// kernel per device — or, where a device index repeats, a host combine.  Raw device pointers of vectors and the expectation communicator
// are not available with a device list (they name ONE device).
//
// The reference has one device index (RandomVariableCuda.java:161,177).  UNMEASURED on more than one physical GPU: the boxes this was
// built on have one; tests use the device lists {0, 0} and {0, 0, 0} — shards on separate streams of one device.
#pragma once
#include <cstdint>
#include <functional>
#include "../../include/fmhip.h"

namespace fm {
// true when a device list is active AND the calling thread is a caller's (not a shard's worker): the C-ABI entry points then hand
// over to the functions below (same signatures and statuses as their fmhip_* namesakes)
bool front_active();
void shard_range(int64_t n, int shards, int shard, int64_t* offset, int64_t* count);
// one order-statistics pass on the calling thread's engine (abi.cpp; a shard's worker calls them), and the bounds bookkeeping both callers share
int os_local_hist(const fmhip_vec* v, int count, int S, const uint32_t* slots, uint32_t shift, uint64_t* hist);
int os_local_sum(const fmhip_vec* v, int count, const uint32_t* keys, double* sums);
int os_local_count(fmhip_vec v, const double* ascending, int m, uint64_t* counts);
// the cross moments of the calling thread's engine (abi.cpp; a shard's worker calls it)
int xmom_local(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums);
int xmom_wide_local(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums);
int xmom_poly_local(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, double* sums);
// the binned cross moments of the calling thread's engine (abi.cpp; a shard's worker calls it)
int binned_xmom_local(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, int64_t* counts, double* sums);
// the kernel moments of the calling thread's engine (abi.cpp; a shard's worker calls it)
int kernel_moments_local(fmhip_vec key, const double* points, const double* bandwidths, int n_points, int kernel, int order, const fmhip_vec* y, int n_y, double* sums);
void os_counts_from_passes(const double* bounds, int n_bounds, int64_t* counts_out, const std::function<void(const double*, int, uint64_t*)>& pass);
namespace front {
int init_devices(const int* devices, int count);
int shutdown();
int device_info(char* name_buf, int name_buf_len, int* n_compute_units, int64_t* hbm_bytes);
int device_count(int* count);
int synchronize();
int vec_create_from_host(const void* host_values, bool is_double, int64_t n, fmhip_vec* out);
int vec_create_filled(int64_t n, double value, bool initialised, fmhip_vec* out);
int vec_retain(fmhip_vec v);
int vec_release(fmhip_vec v);
int vec_size(fmhip_vec v, int64_t* n_out);
int vec_read(fmhip_vec v, void* host_out, bool as_double, int64_t n);
int call(int opcode, int n_in, const fmhip_vec* in, double scalar, bool has_scalar, fmhip_vec* out);
int set_int(int what, int value, int* previous);          // what: 0 fusion, 1 hold, 2 step grouping, 3 math mode, 4 jit mode
int flush();
int graph_clone(const fmhip_vec* roots, int n_roots, int n_copies, const fmhip_vec* leaf_from, const fmhip_vec* leaf_to, int n_map, const double* scalars, int n_scalars, fmhip_vec* out);
int graph_scalars(const fmhip_vec* roots, int n_roots, double* scalars_out, int capacity, int* n_scalars);
int reduce_moments_batch(const fmhip_vec* vectors, int count, const double* shifts, fmhip_moments* out);
int reduce_moments_batch_begin(const fmhip_vec* vectors, int count, const double* shifts, fmhip_ticket* ticket_out);
int reduce_moments_batch_end(fmhip_ticket ticket, fmhip_moments* out, int count);
int reduce_moments_batch_devices(const fmhip_vec* vectors, int count, const double* shifts, void* const* device_out, int n_devices);
int get_stream_of(int shard, void** stream_out);
int expectation_collective(int* kind, char* why, int why_len);
int vec_give_up_values(const fmhip_vec* vectors, int count);
int select_ranks_batch(const fmhip_vec* vectors, int count, const int64_t* ranks, int n_ranks, double* values_out);
int rank_sums_batch(const fmhip_vec* vectors, int count, int64_t rank_from, int64_t rank_to, double* sums_out);
int count_not_above(fmhip_vec v, const double* bounds, int n_bounds, int64_t* counts_out);
int cross_moments(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out);
int cross_moments_wide(const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, double* sums_out);
int binned_cross_moments(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const fmhip_vec* y, int n_y, int64_t* counts_out, double* sums_out);
int binned_evaluate(fmhip_vec key, const double* bounds, int n_bins, const fmhip_vec* x, int n_x, const double* coefficients, fmhip_vec* out);
int sort_by_key(fmhip_vec key, const fmhip_vec* values, int n_values, fmhip_vec* sorted_key_out, fmhip_vec* sorted_values_out);      // one shard; more: FMHIP_ERR_UNSUPPORTED
int argsort(fmhip_vec key, int64_t* permutation_out);
int rank_scores(fmhip_vec key, fmhip_vec* out);
int vec_read_elements(fmhip_vec v, const int64_t* positions, int count, double* out);
int prefix_sums(fmhip_vec v, int mode, fmhip_vec* out, double* total_out);                     // one shard; more: FMHIP_ERR_UNSUPPORTED
int prefix_sums_at(fmhip_vec v, const int64_t* positions, int count, double* sums_out);
int resample(fmhip_vec weights, int scheme, int64_t m, double offset, fmhip_vec uniforms, const fmhip_vec* values, int n_values, fmhip_vec* values_out,
             fmhip_vec* ancestors_out, double* total_out);                                   // one shard; more: FMHIP_ERR_UNSUPPORTED
int compress(fmhip_vec mask, const fmhip_vec* values, int n_values, fmhip_vec* values_out, fmhip_vec* positions_out, int64_t* count_out);      // one shard; more: FMHIP_ERR_UNSUPPORTED
int expand(fmhip_vec mask, const fmhip_vec* values, int n_values, double fill, fmhip_vec* values_out);
int gather(fmhip_vec index, const fmhip_vec* values, int n_values, fmhip_vec* values_out);
int group_sums(fmhip_vec index, int64_t m, const fmhip_vec* values, int n_values, uint32_t mask, fmhip_vec* counts_out, fmhip_vec* outs, int64_t* ungrouped_out);      // one shard; more: FMHIP_ERR_UNSUPPORTED
int table_apply(fmhip_vec x, const double* knots, int count, const double* coefficients, int n_tables, fmhip_vec* out);      // per shard
int function_apply(fmhip_vec x, const int* kinds, int n_functions, fmhip_vec* out);                                         // per shard
int option_formula(int model, fmhip_vec forward, double forward_scalar, fmhip_vec volatility, double volatility_scalar, fmhip_vec payoff_unit,
                   double payoff_unit_scalar, double maturity, double strike, int outputs, fmhip_vec* out);                 // per shard
int implied_volatility(int model, fmhip_vec price, double price_scalar, fmhip_vec forward, double forward_scalar, fmhip_vec payoff_unit,
                       double payoff_unit_scalar, double maturity, double strike, int outputs, fmhip_vec* out);             // per shard
int transform_option(const double* nodes, int n_nodes, int n_states, fmhip_vec forward, double forward_scalar, const fmhip_vec* states, const double* state_scalars,
                     fmhip_vec payoff_unit, double payoff_unit_scalar, double strike, int outputs, fmhip_vec* out);                  // per shard
int prefix_search(fmhip_vec v, const double* thresholds, int count, int relative, int64_t* positions_out, double* sums_out, double* total_out);
int block_moments(const fmhip_vec* vs, int n_vs, int64_t block, uint32_t mask, fmhip_vec* outs);      // one shard; more: FMHIP_ERR_UNSUPPORTED
int vec_repeat(fmhip_vec v, int64_t each, int64_t times, fmhip_vec* out);
int block_order_statistics(const fmhip_vec* vs, int n_vs, int64_t block, const int64_t* ranks, int n_ranks, const int64_t* range_from, const int64_t* range_to,
                           int n_ranges, fmhip_vec* outs);                                             // one shard; more: FMHIP_ERR_UNSUPPORTED
int block_sort(fmhip_vec v, int64_t block, fmhip_vec* out);
int cross_order_statistics(const fmhip_vec* vs, int n_vs, const int* ranks, int n_ranks, int outputs, fmhip_vec* outs);      // per shard
int cross_select(fmhip_vec index, const fmhip_vec* vs, int n_vs, fmhip_vec* out);                                            // per shard
int kernel_moments(fmhip_vec key, const double* points, const double* bandwidths, int n_points, int kernel, int order, const fmhip_vec* y, int n_y, double* sums_out);      // sums add in shard order
int polynomial_cross_moments(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const fmhip_vec* y, int n_y, double* sums_out);
int polynomial_evaluate(const fmhip_vec* states, int n_states, const uint8_t* exponents, int n_terms, const fmhip_vec* extra_x, int n_extra, const double* coefficients, fmhip_vec* out);
int program_create(const fmhip_prog_op* ops, int n_ops, int n_inputs, const int32_t* out_values, int n_outputs, const int32_t* reduce_values, int n_reduce, fmhip_program* out);
int program_release(fmhip_program p);
int program_shape(fmhip_program p, int* n_inputs, int* n_outputs, int* n_reduce);
int program_tier(fmhip_program p, int* tier, int* vgprs);
int program_run(fmhip_program p, int batch, const fmhip_vec* inputs, fmhip_vec* outputs, bool into, const double* reduce_shift, fmhip_moments* moments);
int jit_wait();
int jit_stats(int64_t* compiled, int64_t* failed, int64_t* pending, double* compile_seconds, int64_t* disk_cache_hits);
int bm_generate(int64_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out);
int bm_generate_mersenne_device(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out);
int increments_generate_device(int32_t seed, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const int32_t* kinds, const double* a, const double* b, fmhip_vec* out);
int bm_generate_sobol_device(int32_t seed, int randomize, int construction, int n_steps, int n_factors, int64_t n_paths, int64_t path_offset, const double* dt, fmhip_vec* out);
int pool(int what);                                        // 0 clean, 1 purge
int pool_stats(fmhip_pool_stats_t* out);
int traffic_stats(int64_t* algorithmic_bytes, int64_t* specialised_launches);
int engine_stats(fmhip_engine_stats_t* out);
int profile_enable(int enabled);
int profile_read(double* kernel_ms_total, int64_t* n_launches);
int unsupported(const char* what);
}
}
