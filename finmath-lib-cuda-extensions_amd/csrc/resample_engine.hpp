// resample_engine.hpp — the engine's side of the device resampling (kernels: resample_kernel.hip; definition and argument
// rules: resample_host.hpp).  A producing pass in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// The prefix sums (§4.17) gave the weighted sample its cumulative weight; this is the step that follows it: the weighted sample becomes an
// equally weighted one without a vector leaving the device — m ancestors drawn from the weights (systematic, stratified, multinomial, or
// the bootstrap's equal weights) and up to 8 state vectors carried along, out[i][j] = values[i][a_j].
//
// A weighted call: the chunk totals and bases in the side-pass scratch, P in fp64 in a pool temporary of 8n bytes that goes back to the
// pool when the call ends, four launches chained on the stream and the one that raises the flag; the total reaches the caller through
// pinned memory as fmhip_prefix_sums' does.  With equal weights: one launch, no scratch, no temporary, total = n.
//
// One engine, one sample, as the prefix sums: a device list of several shards or an expectation communicator of several ranks is
// FMHIP_ERR_UNSUPPORTED (sharded.cpp and below), never the resample of a part.
#include "runtime.hpp"
#include "resample_kernel.h"

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_resample.cpp has the stand-in).
hipError_t launch_resample(const DevResampleArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void resample_check(fmhip_vec weights, int scheme, int64_t m, double offset, fmhip_vec uniforms, const fmhip_vec* values, int n_values, const fmhip_vec* values_out,
                    const fmhip_vec* ancestors_out) {
    pass_as_engine_error([&] { resample_check_scalars(scheme, m, offset, n_values, ancestors_out != nullptr, weights != 0, uniforms != 0); });
    if (n_values > 0 && (!values || !values_out)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "resample: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "resample: values[" + std::to_string(i) + "] is no vector");
}
// … and with the sizes known: n of the sample, n_uniforms of the uniforms (m where the scheme reads none)
void resample_check_sizes(int64_t n, int64_t m, int64_t n_uniforms, bool want_ancestors) {
    pass_as_engine_error([&] { resample_check_size(n, want_ancestors); });
    if (n_uniforms != m) throw Error(FMHIP_ERR_SIZE_MISMATCH, "resample: " + std::to_string(n_uniforms) + " uniforms for " + std::to_string(m) + " outputs");
}
// fmhip_resample_host: the definition, with its complaints as engine errors
void resample_host_checked(const float* weights, int64_t n, int scheme, int64_t m, double offset, const float* uniforms, const float* const* values, int n_values,
                           float* const* values_out, int64_t* ancestors_out, double* total_out) {
    pass_as_engine_error([&] { resample_host(weights, n, scheme, m, offset, uniforms, values, n_values, values_out, ancestors_out, total_out); });
}

void Engine::resample(fmhip_vec weights, int scheme, int64_t m, double offset, fmhip_vec uniforms, const fmhip_vec* values, int n_values, fmhip_vec* values_out,
                      fmhip_vec* ancestors_out, double* total_out) {
    require_init();
    resample_check(weights, scheme, m, offset, uniforms, values, n_values, values_out, ancestors_out);
    // the sample: the weights if there are any, then the companions — one size
    std::vector<fmhip_vec> sample;
    if (weights) sample.push_back(weights);
    sample.insert(sample.end(), values, values + n_values);
    const int64_t n = pass_size(sample.data(), (int)sample.size(), "resample");
    const bool with_uniforms = resample_needs_uniforms(scheme);       // (with SYSTEMATIC the uniforms are not looked at)
    resample_check_sizes(n, m, with_uniforms ? node(uniforms)->n : m, ancestors_out != nullptr);
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, "resample with an expectation communicator of " + std::to_string(comm_world) + " ranks: a carry between the ranks is not built");
    pass_need_kernel(launch_resample != nullptr && launch_sort_done != nullptr, "resample");
    PassHold hold, hold_uniforms;
    pass_prepare(sample.data(), (int)sample.size(), hold, "resample");
    if (with_uniforms) pass_prepare(&uniforms, 1, hold_uniforms, "resample");
    PassOutputs made(this);
    DevResampleArgs a{};
    a.n = (uint32_t)n; a.m = (uint32_t)m; a.chunk_tiles = prefix_chunk_tiles(n); a.scheme = (uint32_t)scheme; a.n_values = (uint32_t)n_values; a.offset = offset;
    a.weights = weights ? hold.ptrs[0] : 0;
    a.uniforms = with_uniforms ? hold_uniforms.ptrs[0] : 0;
    for (int i = 0; i < n_values; ++i) { a.values[i] = hold.ptrs[(size_t)i + (weights ? 1u : 0u)]; a.values_out[i] = made.add(m); }
    if (ancestors_out) a.ancestors_out = made.add(m);
    // the temporary of P: its own guard, back in the pool when the call ends (the flag has arrived by then, or the launch failed)
    struct Temporary { Engine* e; Buffer* b = nullptr; ~Temporary() { if (b) e->buffer_unref(b); } } prefix{ this };
    if (weights) prefix.b = new_buffer(resample_prefix_floats(n));
    // pinned: [the total] [flag]
    char* stage = (char*)ensure_stage(256 + 64);
    double* total_host = reinterpret_cast<double*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + 256);
    *total_host = (double)n;
    if (weights) {
        pass_scratch(pass_up256(8), resample_scratch_bytes(n));
        a.prefix = reinterpret_cast<double*>(prefix.b->ptr); a.scratch = (char*)pass_other_; a.total_host = total_host;
    }
    pass_launch_raising(flag, "resample", [&] { return launch_resample(a, stream_); });
    // weighted: the totals read 4n, the prefixes read 4n and write 8n; the gather reads the uniforms and, per output, a few prefixes and the
    // companions (counted once each) and writes the outputs
    const int64_t n_out = n_values + (ancestors_out ? 1 : 0);
    algorithmic_bytes_ += (weights ? 16 * n + 8 * m : 0) + (with_uniforms ? 4 * m : 0) + 4 * m * n_values + 4 * m * n_out;
    bytes_written_ += 4 * m * n_out;
    fmhip_vec ids[FM_RESAMPLE_MAX_VALUES + 1] = {};
    made.commit(ids);
    for (int i = 0; i < n_values; ++i) values_out[i] = ids[i];
    if (ancestors_out) *ancestors_out = ids[n_values];
    if (total_out) *total_out = *total_host;
}

} // namespace fm
