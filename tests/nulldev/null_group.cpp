// null_group.cpp — TEST-ONLY stand-ins for the launchers of group_kernel.hip, beside the null device of tests/nulldev (null_hip.cpp: device
// memory is host memory, launches compute nothing).  Device memory being host memory here, the stand-ins do the real work phase by phase as
// the kernels do: the keys; then per value vector the fill, every chunk of the sorted sequence scanned on its own (levels 1 … 5 of the
// tree with the head flags) leaving its row where the totals kernel writes it, the serial carry over the rows written where the carry
// kernel writes it, and the apply that reads the bases back, adds them to the run that is open at the chunk's start and stores count and
// outputs at the run tails — with the bound checks of the kernels (key < m before an output is addressed, the path index clamped before a
// value is read).  So the scratch and the padded quads that the 16-byte loads reach are touched (an undersized buffer is an ASan report),
// and the chunk-wise scan with its carry is held against the definition's one recursion by drive_group.cpp.  The order between the keys
// and the scan is launch_sort_pass of null_sort.cpp, which also raises the flag (launch_sort_done).
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../finmath-lib-cuda-extensions_amd/csrc/group_kernel.h"

namespace fm {

namespace {
template <class T> T* at(uint64_t address) { return reinterpret_cast<T*>((uintptr_t)address); }
uint32_t last_of_quads(uint32_t n) { return ((n + 3u) & ~3u) - 1u; }      // storage is padded to 256 bytes: the kernels read whole quads
void touch(uint64_t address, uint32_t n) { (void)*(volatile const uint32_t*)&at<const uint32_t>(address)[last_of_quads(n)]; }
}

hipError_t launch_group_keys(const DevGroupKeysArgs& a, hipStream_t) {
    if (!group_keys_shape_ok(a)) return hipErrorInvalidValue;
    const float* index = at<const float>(a.index);
    uint32_t* key = at<uint32_t>(a.key_out);
    uint32_t* idx = at<uint32_t>(a.idx_out);
    for (uint32_t j = 0; j < a.n; ++j) { key[j] = group_key(index[j], (int64_t)a.m); idx[j] = j; }
    return hipSuccess;
}

hipError_t launch_group_scan(const DevGroupScanArgs& a, hipStream_t) {
    if (!group_scan_shape_ok(a)) return hipErrorInvalidValue;
    const int64_t n = (int64_t)a.n, m = (int64_t)a.m, chunk = prefix_chunk_elems(n);
    const uint32_t blocks = prefix_blocks(n);
    const uint32_t* key = at<const uint32_t>(a.key);
    const uint32_t* perm = at<const uint32_t>(a.perm);
    const float* values = a.values ? at<const float>(a.values) : nullptr;
    touch(a.key, a.n); touch(a.perm, a.n);
    if (values) touch(a.values, a.n);
    float* counts = a.counts_out ? at<float>(a.counts_out) : nullptr;
    const bool sums = a.mode != (uint32_t)FM_GROUP_COUNTS, squares = a.mode == (uint32_t)FM_GROUP_S1_S2;
    // fill
    for (int64_t k = 0; k < m; ++k) {
        if (counts) counts[k] = 0.0f;
        int j = 0;
        for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1) if (a.mask & (uint32_t)bit) at<float>(a.outs[j++])[k] = group_output(bit, 0.0, 0.0, 0);
    }
    std::vector<unsigned char> head((size_t)n);
    for (int64_t r = 0; r < n; ++r) head[(size_t)r] = r == 0 || key[r] != key[r - 1];
    std::vector<double> p1(sums ? (size_t)n : 0), p2(squares ? (size_t)n : 0);
    for (int64_t r = 0; sums && r < n; ++r) {
        const double x = (double)values[perm[r] < a.n ? perm[r] : a.n - 1u];
        p1[(size_t)r] = x;
        if (squares) p2[(size_t)r] = x * x;
    }
    // totals: every chunk on its own
    GroupRow* rows = group_rows(a);
    GroupRow* bases = group_bases(a);
    for (uint32_t c = 0; c < blocks; ++c) {
        const int64_t off = (int64_t)c * chunk, cnt = std::min<int64_t>(chunk, n - off);
        GroupRow row; row.s1 = 0.0; row.s2 = 0.0; row.head = 0u; row.pad = 0u;
        if (sums) { group_unit_host(p1.data() + off, head.data() + off, cnt, 5, chunk); row.s1 = p1[(size_t)(off + cnt - 1)]; }
        if (squares) { group_unit_host(p2.data() + off, head.data() + off, cnt, 5, chunk); row.s2 = p2[(size_t)(off + cnt - 1)]; }
        for (int64_t r = off; r < off + cnt; ++r) if (head[(size_t)r]) row.head = (uint32_t)r + 1u;
        rows[c] = row;
    }
    // carry
    {
        double run1 = rows[0].s1, run2 = rows[0].s2;
        uint32_t start = rows[0].head;
        GroupRow none; none.s1 = 0.0; none.s2 = 0.0; none.head = 0u; none.pad = 0u;
        bases[0] = none;
        for (uint32_t c = 1; c < blocks; ++c) {
            GroupRow b; b.s1 = run1; b.s2 = run2; b.head = start; b.pad = 0u;
            bases[c] = b;
            const bool h = rows[c].head != 0u;
            run1 = h ? rows[c].s1 : run1 + rows[c].s1;
            run2 = h ? rows[c].s2 : run2 + rows[c].s2;
            start = std::max(start, rows[c].head);
        }
    }
    // apply
    for (uint32_t c = 0; c < blocks; ++c) {
        const int64_t off = (int64_t)c * chunk, cnt = std::min<int64_t>(chunk, n - off);
        const GroupRow base = bases[c];
        uint32_t start = base.head;
        bool open = true;
        for (int64_t r = off; r < off + cnt; ++r) {
            const uint32_t k = key[r];
            if (head[(size_t)r]) { start = (uint32_t)r + 1u; open = false; }
            if (a.ungrouped_host && head[(size_t)r] && k >= a.m) *a.ungrouped_host = (uint64_t)(n - r);
            const bool tail = r == n - 1 || key[r + 1] != k;
            if (!tail || k >= a.m) continue;
            if (a.ungrouped_host && r == n - 1) *a.ungrouped_host = 0u;                // every element grouped: the tail at n - 1 says so
            const int64_t count = r + 2 - (int64_t)start;
            if (counts) counts[k] = (float)count;
            if (!sums) continue;
            const bool add = c > 0u && open;
            const double S1 = add ? base.s1 + p1[(size_t)r] : p1[(size_t)r];
            const double S2 = !squares ? 0.0 : add ? base.s2 + p2[(size_t)r] : p2[(size_t)r];
            int j = 0;
            for (int bit = 1; bit <= fmhost::FM_BLOCK_VARIANCE; bit <<= 1) if (a.mask & (uint32_t)bit) at<float>(a.outs[j++])[k] = group_output(bit, S1, S2, count);
        }
    }
    return hipSuccess;
}

} // namespace fm
