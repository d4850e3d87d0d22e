// sort_engine.hpp — the engine's side of the device sort (kernels: sort_kernel.hip; definition and chunk arithmetic:
// sort_host.hpp).  Passes in the frame of side_pass_engine.hpp (which says what every such pass does).
//
// The reference downloads a vector and sorts it on the host whenever it needs more than a few ranks: the whole ordered sample, the
// permutation, ranks per path.  Here the vector stays where it is: a stable radix sort of (key, path index) pairs leaves the permutation in
// pool storage, and one more kernel turns it into what the call wants — the key and its companions gathered (sort_by_key), the permutation
// itself (argsort), the rank scores scattered back to the paths (rank_scores).  read_elements is the other half of a quantile table: a few
// elements of a vector into pinned memory, not the vector.
//
// Every call: the count table in the side-pass scratch, one chain of launches that raises the flag and is waited for.  The four ping-pong
// buffers (16·n bytes) come from the pool like vector storage, BEFORE the outputs, and are back in it when the call returns.
//
// One engine, one sample: the order of a sample that is spread over the shards of a device list or the ranks of an expectation communicator
// needs an exchange of ELEMENTS, which nothing here does — such a call is FMHIP_ERR_UNSUPPORTED (abi.cpp, sharded.cpp and below), never
// the order of a part.
#include "runtime.hpp"
#include "sort_kernel.h"

#include <cstring>

namespace fm {

// WEAK: see pass_need_kernel (launch_sort_done, which these share with every chain that raises the flag, is declared by the frame).
hipError_t launch_sort_pass(const DevSortPassArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_sort_gather(const DevSortGatherArgs& a, hipStream_t st) __attribute__((weak));
hipError_t launch_sort_scores(uint64_t perm, uint64_t out, uint32_t n, hipStream_t st) __attribute__((weak));
hipError_t launch_sort_read_elements(uint64_t v, const uint32_t* pos, uint32_t count, double* out_host, hipStream_t st) __attribute__((weak));

// what can be said about the arguments without looking at a vector: FMHIP_ERR_INVALID_ARGUMENT
void sort_check_by_key(fmhip_vec key, const fmhip_vec* values, int n_values, const fmhip_vec* sorted_key_out, const fmhip_vec* sorted_values_out) {
    if (!key) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "sort by key: the key is a vector");
    if (n_values < 0 || n_values > FM_SORT_MAX_VALUES) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "sort by key: " + std::to_string(n_values) + " companion vectors (0 … " + std::to_string(FM_SORT_MAX_VALUES) + ")");
    if (n_values > 0 && (!values || !sorted_values_out)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "sort by key: null pointer: values");
    if (n_values == 0 && !sorted_key_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "sort by key: nothing is asked for");
    for (int i = 0; i < n_values; ++i) if (!values[i]) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "sort by key: a companion is a vector");
}
void sort_check_read_elements(fmhip_vec v, const int64_t* positions, int count, const double* out) {
    if (!v) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "read elements: of a vector");
    if (count < 1) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "read elements: count must be positive");
    if (!positions || !out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "read elements: null pointer");
}
// fmhip_argsort_host: the definition, with its complaints as engine errors
void sort_argsort_host_checked(const float* key, int64_t n, int64_t* permutation_out) {
    pass_as_engine_error([&] { sort_argsort_host(key, n, permutation_out); });
}

// The ping-pong buffers of a sort, from the pool, back in it when the call ends — however it ends.
struct Engine::SortBuffers {
    Engine* e;
    Buffer* b[4] = { nullptr, nullptr, nullptr, nullptr };       // key A, index A, key B, index B
    SortBuffers(Engine* eng, int64_t n) : e(eng) { try { for (Buffer*& x : b) x = e->new_buffer(n); } catch (...) { drop(); throw; } }
    ~SortBuffers() { drop(); }
    void drop() { for (Buffer*& x : b) if (x) { e->buffer_unref(x); x = nullptr; } }
    uint64_t at(int i) const { return (uint64_t)(uintptr_t)b[i]->ptr; }
};

// the size of a sort's sample, or the refusals that need no look at the values: before anything is flushed or launched
int64_t Engine::sort_size(const fmhip_vec* hs, int count, const char* what) {
    const int64_t n = pass_size(hs, count, what);
    if (!sort_size_ok(n)) throw Error(FMHIP_ERR_INVALID_ARGUMENT, std::string(what) + " of " + std::to_string(n) + " elements: at most 2^31 - 1");
    if (comm_world > 1) throw Error(FMHIP_ERR_UNSUPPORTED, std::string(what) + " with an expectation communicator of " + std::to_string(comm_world) + " ranks: a global order needs an exchange of elements between the ranks");
    pass_need_kernel(launch_sort_pass != nullptr && launch_sort_gather != nullptr && launch_sort_scores != nullptr && launch_sort_done != nullptr, "sort");
    return n;
}

// The four passes, enqueued; the permutation is in index buffer B behind them.  key_ptr: the float vector.
hipError_t Engine::sort_enqueue(uint64_t key_ptr, int64_t n, const SortBuffers& s) {
    DevSortPassArgs a{};
    a.n = (uint32_t)n; a.chunk_tiles = sort_chunk_tiles(n);
    a.table = (uint32_t*)pass_other_;
    for (int pass = 0; pass < FM_SORT_PASSES; ++pass) {
        const int from = (pass & 1) ? 0 : 2, to = (pass & 1) ? 2 : 0;       // pass 0: vector → A; 1: A → B; 2: B → A; 3: A → B
        a.shift = 8u * (uint32_t)pass;
        a.from_floats = pass == 0; a.write_keys = pass != FM_SORT_PASSES - 1;
        a.src_key = pass == 0 ? key_ptr : s.at(from); a.src_idx = pass == 0 ? 0 : s.at(from + 1);
        a.dst_key = s.at(to); a.dst_idx = s.at(to + 1);
        const hipError_t e = launch_sort_pass(a, stream_);
        if (e != hipSuccess) return e;
    }
    // per pass: the count reads 4n, the scatter reads 8n and writes 8n; the first pass reads no indices, the last writes no keys
    algorithmic_bytes_ += (int64_t)FM_SORT_PASSES * 20 * n - 8 * n;
    return hipSuccess;
}
static_assert(FM_SORT_PASSES == 4, "sort_enqueue leaves the permutation in index buffer B after an even number of passes");

void Engine::sort_by_key(fmhip_vec key, const fmhip_vec* values, int n_values, fmhip_vec* sorted_key_out, fmhip_vec* sorted_values_out) {
    require_init();
    sort_check_by_key(key, values, n_values, sorted_key_out, sorted_values_out);
    fmhip_vec all[1 + FM_SORT_MAX_VALUES];
    all[0] = key;
    for (int i = 0; i < n_values; ++i) all[1 + i] = values[i];
    const int64_t n = sort_size(all, 1 + n_values, "sort by key");
    PassHold hold;
    pass_prepare(all, 1 + n_values, hold, "sort by key");
    SortBuffers s(this, n);
    // the outputs, in the order of the gather's list: the key if it is asked for, then the companions
    PassOutputs outs(this);
    DevSortGatherArgs g{};
    g.n = (uint32_t)n; g.perm = s.at(3);
    for (int i = sorted_key_out ? 0 : 1; i < 1 + n_values; ++i) {
        g.src[g.count] = hold.ptrs[(size_t)i];
        g.dst[g.count++] = outs.add(n);
    }
    char* stage = (char*)ensure_stage(64);
    pass_scratch(pass_up256(8), sort_table_bytes(n));
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "sort by key", [&] {
        const hipError_t e = sort_enqueue(hold.ptrs[0], n, s);
        return e == hipSuccess ? launch_sort_gather(g, stream_) : e;
    });
    algorithmic_bytes_ += 4 * n + 8 * n * (int64_t)g.count;
    bytes_written_ += 4 * n * (int64_t)g.count;
    outs.commit(sorted_values_out, sorted_key_out);
}

void Engine::argsort(fmhip_vec key, int64_t* permutation_out) {
    require_init();
    if (!key || !permutation_out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "argsort: of a vector, into a host array");
    const int64_t n = sort_size(&key, 1, "argsort");
    PassHold hold;
    pass_prepare(&key, 1, hold, "argsort");
    SortBuffers s(this, n);
    char* stage = (char*)ensure_stage(64);
    pass_scratch(pass_up256(8), sort_table_bytes(n));
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "argsort", [&] { return sort_enqueue(hold.ptrs[0], n, s); });
    // the permutation comes down as read() brings a vector down: through the pinned block, widened on the way
    const uint32_t* perm = reinterpret_cast<const uint32_t*>(s.b[3]->ptr);
    const int64_t chunk = FM_SORT_READBACK_CHUNK;
    for (int64_t off = 0; off < n; off += chunk) {
        const int64_t m = std::min(chunk, n - off);
        uint32_t* st = (uint32_t*)ensure_stage((size_t)m * 4);
        hip_check(hipMemcpyAsync(st, perm + off, (size_t)m * 4, hipMemcpyDeviceToHost, stream_), "D2H(permutation)");
        wait_for_stream("D2H sync");
        for (int64_t i = 0; i < m; ++i) permutation_out[off + i] = (int64_t)st[i];
    }
}

void Engine::rank_scores(fmhip_vec key, fmhip_vec* out) {
    require_init();
    if (!key || !out) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "rank scores: of a vector, into a handle");
    const int64_t n = sort_size(&key, 1, "rank scores");
    PassHold hold;
    pass_prepare(&key, 1, hold, "rank scores");
    SortBuffers s(this, n);
    PassOutputs outs(this);
    const uint64_t scores = outs.add(n);
    char* stage = (char*)ensure_stage(64);
    pass_scratch(pass_up256(8), sort_table_bytes(n));
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage);
    pass_launch_raising(flag, "rank scores", [&] {
        const hipError_t e = sort_enqueue(hold.ptrs[0], n, s);
        return e == hipSuccess ? launch_sort_scores(s.at(3), scores, (uint32_t)n, stream_) : e;
    });
    algorithmic_bytes_ += 8 * n;
    bytes_written_ += 4 * n;
    outs.commit(out);
}

void Engine::read_elements(fmhip_vec v, const int64_t* positions, int count, double* out) {
    require_init();
    sort_check_read_elements(v, positions, count, out);
    const int64_t n = pass_size(&v, 1, "read elements");
    for (int j = 0; j < count; ++j)
        if (positions[j] < 0 || positions[j] >= n) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "position " + std::to_string(positions[j]) + " outside a vector of " + std::to_string(n));
    if (n > FM_SORT_MAX_N) throw Error(FMHIP_ERR_INVALID_ARGUMENT, "read elements of a vector of more than 2^31 - 1 elements");
    pass_need_kernel(launch_sort_read_elements != nullptr && launch_sort_done != nullptr, "read-elements");
    PassHold hold;
    pass_prepare(&v, 1, hold, "read elements");
    // pinned: [positions (copied to the device in-stream)] [the elements] [flag]
    const size_t tab_bytes = pass_up256((size_t)count * 4), out_bytes = pass_up256((size_t)count * 8);
    char* stage = (char*)ensure_stage(tab_bytes + out_bytes + 64);
    pass_scratch(pass_up256(8), tab_bytes);
    uint32_t* pos_host = reinterpret_cast<uint32_t*>(stage);
    double* out_host = reinterpret_cast<double*>(stage + tab_bytes);
    volatile uint64_t* flag = reinterpret_cast<volatile uint64_t*>(stage + tab_bytes + out_bytes);
    for (int j = 0; j < count; ++j) pos_host[j] = (uint32_t)positions[j];
    hip_check(hipMemcpyAsync(pass_other_, stage, tab_bytes, hipMemcpyHostToDevice, stream_), "H2D(positions)");
    pass_launch_raising(flag, "read elements", [&] { return launch_sort_read_elements(hold.ptrs[0], (const uint32_t*)pass_other_, (uint32_t)count, out_host, stream_); });
    for (int j = 0; j < count; ++j) out[j] = out_host[j];
}

} // namespace fm
