// group_engine.hpp — the engine's side of the device reduce-by-key (kernels: group_kernel.hip; definition and argument
// rules: group_host.hpp).  A producing pass in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// What no pass before could do: aggregate by an integer vector that another pass left on the device — the ancestors of a resample, the slot
// of an argmax, a bin number, a Poisson count.  out[k] = Σ { v[j] : index[j] == k } for up to four value vectors, as sum, mean and variance
// per group, with the count per group and the number of elements that belong to no group.
//
// ONE chain, one wait: keys → one to four radix passes (the sort's, from the ready pair) → per value vector fill, totals, carry, apply.
// The outputs have m elements, which the caller names: they are allocated through PassOutputs before anything is launched, the temporaries
// (two key buffers, two index buffers: the sort's ping-pong) come from the pool and go back when the call ends, however it ends.  The
// number of ungrouped elements reaches the host through pinned memory beside the flag.  The value vectors are sliced over the scan launches
// one by one: the definition makes a group's bits independent of that.
//
// One engine, one sample: a device list of several shards or an expectation communicator of several ranks is FMHIP_ERR_UNSUPPORTED
// (sharded.cpp and below) — a group's members lie on every shard, and the association over shards is not the definition's.
#include "runtime.hpp"
#include "group_kernel.h"

namespace fm {

// WEAK: see pass_need_kernel (tests/nulldev/null_group.cpp has the stand-ins).
hipError_t launch_group_keys(const DevGroupKeysArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_group_scan(const DevGroupScanArgs& a, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void group_check(fmhip_vec index, int64_t m, const fmhip_vec* values, int n_values, uint32_t mask, const fmhip_vec* counts_out, const fmhip_vec* outs, const int64_t* ungrouped_out) {
    pass_as_engine_error([&] { group_check_scalars(m, n_values, mask, counts_out != nullptr || ungrouped_out != nullptr); });
    if (!index) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "group sums: the index is no vector");
    if (n_values > 0 && (!values || !outs)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "group sums: null pointer");
    for (int i = 0; i < n_values; ++i) if (!values[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "group sums: values[" + std::to_string(i) + "] is no vector");
}
// … and with the size of the index known
void group_check_index_size(int64_t n) {
    pass_as_engine_error([&] { group_check_size(n); });
}
// fmhip_group_sums_host: the definition, with its complaints as engine errors
void group_sums_host_checked(const float* index, int64_t n, int64_t m, const float* const* values, int n_values, uint32_t mask, float* counts_out, float* const* outs, int64_t* ungrouped_out) {
    pass_as_engine_error([&] { group_sums_host(index, n, m, values, n_values, mask, counts_out, outs, ungrouped_out); });
}

void Engine::group_sums(fmhip_vec index, int64_t m, const fmhip_vec* values, int n_values, uint32_t mask, fmhip_vec* counts_out, fmhip_vec* outs, int64_t* ungrouped_out) {
    require_init();
    group_check(index, m, values, n_values, mask, counts_out, outs, ungrouped_out);
    std::vector<fmhip_vec> sample{ index };
    sample.insert(sample.end(), values, values + n_values);
    const int64_t n = pass_size(sample.data(), (int)sample.size(), "group sums");
    group_check_index_size(n);
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, "group sums with an expectation communicator of " + std::to_string(comm_world) + " ranks: an exchange between the ranks is not built");
    pass_need_kernel(launch_group_keys != nullptr && launch_group_scan != nullptr && launch_sort_pass != nullptr && launch_sort_done != nullptr, "group sums");
    PassHold hold;
    pass_prepare(sample.data(), (int)sample.size(), hold, "group sums");
    SortBuffers s(this, n);
    PassOutputs made(this);
    const int per = fmhost::fm_block_outputs(mask);
    const uint64_t counts = counts_out ? made.add(m) : 0;
    uint64_t out_ptrs[FM_GROUP_MAX_VALUES * fmhost::FM_BLOCK_MAX_OUTPUTS] = {};
    for (int i = 0; i < n_values * per; ++i) out_ptrs[i] = made.add(m);
    char* stage = (char*)ensure_stage(256 + 64);                  // pinned: [the number of ungrouped elements] [flag]
    uint64_t* ungrouped_host = reinterpret_cast<uint64_t*>(stage);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + 256);
    *ungrouped_host = ~uint64_t(0);                               // the apply kernel writes it whatever the index holds: 0 where every element is grouped
    pass_scratch(pass_up256(8), group_scratch_bytes(n));
    const int passes = group_sort_passes(m);
    const int sorted = (passes & 1) ? 2 : 0;                     // pass 0: A → B; 1: B → A; 2: A → B; 3: B → A
    pass_launch_raising(flag, "group sums", [&] {
        DevGroupKeysArgs k{};
        k.n = (uint32_t)n; k.m = (uint32_t)m; k.index = hold.ptrs[0]; k.key_out = s.at(0); k.idx_out = s.at(1);
        hipError_t e = launch_group_keys(k, stream_);
        DevSortPassArgs p{};
        p.n = (uint32_t)n; p.chunk_tiles = sort_chunk_tiles(n); p.table = (uint32_t*)pass_other_; p.from_floats = 0; p.write_keys = 1;
        for (int pass = 0; pass < passes && e == hipSuccess; ++pass) {
            const int from = (pass & 1) ? 2 : 0, to = (pass & 1) ? 0 : 2;
            p.shift = 8u * (uint32_t)pass;
            p.src_key = s.at(from); p.src_idx = s.at(from + 1); p.dst_key = s.at(to); p.dst_idx = s.at(to + 1);
            e = launch_sort_pass(p, stream_);
        }
        DevGroupScanArgs a{};
        a.n = (uint32_t)n; a.m = (uint32_t)m; a.chunk_tiles = prefix_chunk_tiles(n); a.key = s.at(sorted); a.perm = s.at(sorted + 1);
        a.scratch = (char*)pass_other_ + group_table_bytes(n);
        // the first launch leaves the counts and the number of ungrouped elements; a call without value vectors is that launch alone
        for (int i = 0; i < (n_values > 0 ? n_values : 1) && e == hipSuccess; ++i) {
            a.counts_out = i == 0 ? counts : 0;
            a.ungrouped_host = i == 0 ? ungrouped_host : nullptr;
            if (n_values > 0) {
                a.mode = (mask & (uint32_t)fmhost::FM_BLOCK_VARIANCE) ? (uint32_t)FM_GROUP_S1_S2 : (uint32_t)FM_GROUP_S1;
                a.mask = mask; a.values = hold.ptrs[(size_t)i + 1];
                for (int j = 0; j < per; ++j) a.outs[j] = out_ptrs[i * per + j];
            } else a.mode = (uint32_t)FM_GROUP_COUNTS;
            e = launch_group_scan(a, stream_);
        }
        return e;
    });
    const uint64_t ungrouped = *ungrouped_host;
    if (ungrouped > (uint64_t)n) throw Error(FMHIP_ERR_HIP, "the group sums ended without delivering the number of ungrouped elements");
    // the keys: 4n read, 8n written; a radix pass: the count reads 4n, the scatter reads 8n and writes 8n; a scan reads the pair and the
    // values twice (totals and apply) and writes its outputs twice (fill and apply)
    const int64_t scans = n_values > 0 ? n_values : 1, n_out = (int64_t)n_values * per + (counts_out ? 1 : 0);
    algorithmic_bytes_ += 12 * n + (int64_t)passes * 20 * n + scans * 2 * (8 * n + (n_values > 0 ? 8 * n : 0)) + 8 * m * n_out;
    bytes_written_ += 4 * m * n_out;
    if (n_out > 0) made.commit(outs, counts_out);
    if (ungrouped_out) *ungrouped_out = (int64_t)ungrouped;
}

} // namespace fm
