// test_select_host.cpp — the definition of the device selection (csrc/select_host.hpp) on the CPU, built with -fsanitize=address,undefined
// by tests/test_select_cpu.py: compress, expand and gather against a plain restatement over every mask family at sizes around every
// boundary of the chunk geometry, with exactly-sized heap arrays (a compress writes `count` elements and not one more; the arrays of an
// expand have `count` elements and not one more); a MODEL of the kernels as they run — chunk counts, exclusive bases, the bits of a lane's
// eight elements, the scan inside the tile, the bound checks — whose every output must be the definition's, also with a WRONG count; the
// decoding of an index on hostile values; every refusal.
#include "../../finmath-lib-cuda-extensions_amd/csrc/select_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

using namespace fm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)
template <class F> static bool refuses(F f) { try { f(); } catch (const std::invalid_argument&) { return true; } return false; }

static const int FAMILIES = 9;
static std::vector<float> mask_of(int64_t n, int family, std::mt19937& rng)
{
    std::vector<float> m((size_t)n);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    const float odd[6] = { std::numeric_limits<float>::quiet_NaN(), -0.f, 0.f, -1e-45f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity() };
    for (int64_t p = 0; p < n; ++p) {
        float x;
        switch (family) {
        case 0: x = 1.f; break;
        case 1: x = -1.f; break;
        case 2: x = p == 0 ? 0.f : -1.f; break;
        case 3: x = p == n - 1 ? 2.f : -2.f; break;
        case 4: x = (p & 1) ? 1.f : -1.f; break;
        case 5: x = p % 64 == 17 % (n < 64 ? n : 64) ? 1.f : -1.f; break;
        case 6: x = uni(rng) - 0.5f; break;
        case 7: x = uni(rng) - 0.99f; break;
        default: x = odd[rng() % 6u];
        }
        m[(size_t)p] = x;
    }
    return m;
}
static std::vector<float> values_of(int64_t n, uint32_t seed)
{
    std::vector<float> v((size_t)n);
    for (int64_t p = 0; p < n; ++p) {
        uint32_t bits = (uint32_t)p * 2654435761u + seed;
        if (p % 7 == 1) bits = 0x7fc01234u + (uint32_t)(p & 0xff);      // NaNs with payloads
        if (p % 7 == 3) bits = 0x80000000u;                             // -0.0
        std::memcpy(&v[(size_t)p], &bits, 4);
    }
    return v;
}
static bool same(const float* a, const float* b, int64_t count) { return count == 0 || std::memcmp(a, b, (size_t)count * 4) == 0; }

// the kernels as they run: the chunk counts and bases, then per tile and lane the bits, the scan and the checked stores
static void kernel_model(const std::vector<float>& mask, const std::vector<float>& v, uint32_t allocated, std::vector<float>& out, std::vector<float>& positions,
                         std::vector<float>& expanded, const std::vector<float>& short_v, float fill, uint32_t& count)
{
    const int64_t n = (int64_t)mask.size(), chunk = prefix_chunk_elems(n);
    const uint32_t blocks = prefix_blocks(n);
    std::vector<uint32_t> counts(blocks, 0u), bases(blocks + 1u, 0u);
    for (uint32_t c = 0; c < blocks; ++c)
        for (int64_t r = (int64_t)c * chunk; r < n && r < (int64_t)(c + 1) * chunk; ++r) counts[c] += select_selected(mask[(size_t)r]) ? 1u : 0u;
    for (uint32_t c = 0; c < blocks; ++c) bases[c + 1u] = bases[c] + counts[c];
    count = bases[blocks];
    out.assign(allocated, -7.f); positions.assign(allocated, -7.f); expanded.assign((size_t)n, -7.f);
    for (uint32_t c = 0; c < blocks; ++c) {
        uint32_t run = bases[c];
        for (int64_t tile = (int64_t)c * prefix_chunk_tiles(n); tile < (int64_t)(c + 1) * prefix_chunk_tiles(n) && tile < prefix_tiles(n); ++tile) {
            uint32_t lane_base = run;
            for (int lane = 0; lane < FM_PREFIX_BLOCK; ++lane) {
                const int64_t e0 = tile * FM_PREFIX_TILE + (int64_t)lane * FM_PREFIX_ITEMS;
                uint32_t bits = 0u;
                for (int i = 0; i < FM_PREFIX_ITEMS; ++i) if (e0 + i < n && select_selected(mask[(size_t)(e0 + i)])) bits |= 1u << i;
                for (int i = 0; i < FM_PREFIX_ITEMS; ++i) {
                    const uint32_t q = lane_base + (uint32_t)__builtin_popcount(bits & ((1u << i) - 1u));
                    if ((bits >> i & 1u) && q < allocated) { out[q] = v[(size_t)(e0 + i)]; positions[q] = (float)(e0 + i); }
                    if (e0 + i < n && !short_v.empty()) {
                        const uint32_t last = (uint32_t)short_v.size() - 1u;
                        const float x = short_v[q < last ? q : last];
                        expanded[(size_t)(e0 + i)] = (bits >> i & 1u) ? x : fill;
                    }
                }
                lane_base += (uint32_t)__builtin_popcount(bits);
            }
            run = lane_base;
        }
    }
}

static void one_size(int64_t n, std::mt19937& rng)
{
    const std::vector<float> v = values_of(n, 17u), v2 = values_of(n, 99u);
    for (int family = 0; family < FAMILIES; ++family) {
        const std::vector<float> mask = mask_of(n, family, rng);
        std::vector<int64_t> sel;
        for (int64_t r = 0; r < n; ++r) if (mask[(size_t)r] >= 0.0f) sel.push_back(r);
        const int64_t want = (int64_t)sel.size();
        CHECK(select_count_host(mask.data(), n) == want);
        // compress into arrays of capacity n, then into exactly-sized ones through the kernels' model
        std::vector<float> o1((size_t)n, -7.f), o2((size_t)n, -7.f);
        std::vector<int64_t> pos((size_t)n, -7);
        const float* in[2] = { v.data(), v2.data() }; float* columns[2] = { o1.data(), o2.data() };
        int64_t count = -1;
        compress_host(mask.data(), n, in, 2, columns, pos.data(), &count);
        CHECK(count == want);
        for (int64_t q = 0; q < want; ++q) CHECK(pos[(size_t)q] == sel[(size_t)q] && same(&o1[(size_t)q], &v[(size_t)sel[(size_t)q]], 1) && same(&o2[(size_t)q], &v2[(size_t)sel[(size_t)q]], 1));
        for (int64_t q = want; q < n; ++q) CHECK(pos[(size_t)q] == -7 && o1[(size_t)q] == -7.f);
        int64_t only = -1;
        compress_host(mask.data(), n, nullptr, 0, nullptr, nullptr, &only);
        CHECK(only == want);
        // expand back
        for (float fill : { 0.f, -0.f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN() }) {
            std::vector<float> shorter(o1.begin(), o1.begin() + want), e((size_t)n, -7.f);
            if (shorter.empty()) shorter.push_back(0.f);
            const float* sin[1] = { shorter.data() }; float* eout[1] = { e.data() };
            CHECK(expand_host(mask.data(), n, sin, 1, want, (double)fill, eout));
            for (int64_t r = 0; r < n; ++r) CHECK(same(&e[(size_t)r], mask[(size_t)r] >= 0.0f ? &v[(size_t)r] : &fill, 1));
            std::vector<float> untouched((size_t)n, -7.f); float* uout[1] = { untouched.data() };
            CHECK(!expand_host(mask.data(), n, sin, 1, want + 1, (double)fill, uout) && untouched[0] == -7.f && untouched[(size_t)n - 1] == -7.f);
        }
        // gather by the positions is the compress
        if (want > 0) {
            std::vector<float> index((size_t)want), g((size_t)want, -7.f);
            for (int64_t q = 0; q < want; ++q) index[(size_t)q] = (float)sel[(size_t)q];
            const float* gin[1] = { v.data() }; float* gout[1] = { g.data() };
            gather_host(index.data(), want, gin, 1, n, gout);
            CHECK(same(g.data(), o1.data(), want));
        }
        // the kernels' model: with the right count, with a count that is too small and with one that is too large
        for (int64_t allocated : { want, want / 2, want + 3 }) {
            if (allocated <= 0) continue;
            std::vector<float> out, positions, expanded, shorter(o1.begin(), o1.begin() + std::min(want, allocated));
            if (shorter.empty()) shorter.push_back(0.f);
            uint32_t got = 0;
            kernel_model(mask, v, (uint32_t)allocated, out, positions, expanded, shorter, 3.5f, got);
            CHECK((int64_t)got == want);
            const int64_t upto = std::min(want, allocated);
            CHECK(same(out.data(), o1.data(), upto));
            for (int64_t q = 0; q < upto; ++q) CHECK(positions[(size_t)q] == (float)sel[(size_t)q]);
            for (int64_t q = upto; q < allocated; ++q) CHECK(out[(size_t)q] == -7.f);
            if (allocated == want) for (int64_t r = 0; r < n; ++r) { const float f = 3.5f; CHECK(same(&expanded[(size_t)r], mask[(size_t)r] >= 0.0f ? &v[(size_t)r] : &f, 1)); }
        }
    }
}

static void indices()
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    CHECK(select_index(-1.f, 10) == -1 && select_index(-0.f, 10) == 0 && select_index(0.f, 10) == 0 && select_index(9.f, 10) == 9 && select_index(10.f, 10) == -1);
    CHECK(select_index(0.5f, 10) == -1 && select_index(nan, 10) == -1 && select_index(inf, 10) == -1 && select_index(-inf, 10) == -1 && select_index(-1e-45f, 10) == -1);
    CHECK(select_index(3e38f, FM_PREFIX_MAX_N) == -1 && select_index(2147483648.f, FM_PREFIX_MAX_N) == -1 && select_index(2147483520.f, FM_PREFIX_MAX_N) == 2147483520LL);
    const int64_t big = (int64_t(1) << 24) + 2;                        // n - 1 = 2^24 + 1 is no float: the comparison is made in double
    CHECK(select_index((float)big, big) == -1 && select_index((float)(big - 2), big) == big - 2 && select_index((float)big, big + 1) == big);
    const float v[3] = { 1.f, 2.f, 3.f }, index[8] = { -1.f, -0.f, 2.f, 3.f, 0.5f, nan, inf, -inf };
    float out[8]; const float* in[1] = { v }; float* columns[1] = { out };
    gather_host(index, 8, in, 1, 3, columns);
    uint32_t bits[8]; std::memcpy(bits, out, 32);
    CHECK(bits[0] == FM_SELECT_NAN_BITS && out[1] == 1.f && out[2] == 3.f);
    for (int j = 3; j < 8; ++j) CHECK(bits[j] == FM_SELECT_NAN_BITS);
    CHECK(select_selected(0.f) && select_selected(-0.f) && select_selected(inf) && !select_selected(nan) && !select_selected(-1e-45f) && !select_selected(-inf));
}

static void refusals()
{
    const float m[4] = { 1.f, -1.f, 1.f, 1.f }, v[4] = { 1.f, 2.f, 3.f, 4.f };
    float o[4]; int64_t pos[4], count = -7;
    const float* in[9] = { v, v, v, v, v, v, v, v, v }; float* out[9] = { o, o, o, o, o, o, o, o, o };
    const float* holed[1] = { nullptr };
    CHECK(refuses([&] { compress_host(m, 4, in, 9, out, pos, &count); }) && refuses([&] { compress_host(m, 4, in, -1, out, pos, &count); }));
    CHECK(refuses([&] { compress_host(m, 0, in, 1, out, pos, &count); }) && refuses([&] { compress_host(m, int64_t(1) << 31, in, 1, out, pos, &count); }));
    CHECK(refuses([&] { compress_host(m, (int64_t(1) << 24) + 1, in, 1, out, pos, &count); }));
    CHECK(refuses([&] { compress_host(nullptr, 4, in, 1, out, pos, &count); }) && refuses([&] { compress_host(m, 4, nullptr, 1, out, pos, &count); }));
    CHECK(refuses([&] { compress_host(m, 4, in, 1, nullptr, pos, &count); }) && refuses([&] { compress_host(m, 4, holed, 1, out, pos, &count); }));
    CHECK(refuses([&] { expand_host(m, 4, in, 0, 3, 0.0, out); }) && refuses([&] { expand_host(m, 4, in, 9, 3, 0.0, out); }) && refuses([&] { expand_host(m, 0, in, 1, 3, 0.0, out); }));
    CHECK(refuses([&] { expand_host(nullptr, 4, in, 1, 3, 0.0, out); }) && refuses([&] { expand_host(m, 4, nullptr, 1, 3, 0.0, out); }) && refuses([&] { expand_host(m, 4, holed, 1, 3, 0.0, out); }));
    CHECK(refuses([&] { gather_host(m, 4, in, 0, 4, out); }) && refuses([&] { gather_host(m, 4, in, 9, 4, out); }) && refuses([&] { gather_host(m, 0, in, 1, 4, out); }));
    CHECK(refuses([&] { gather_host(m, 4, in, 1, 0, out); }) && refuses([&] { gather_host(nullptr, 4, in, 1, 4, out); }) && refuses([&] { gather_host(m, 4, holed, 1, 4, out); }));
    CHECK(count == -7);
}

int main()
{
    std::mt19937 rng(20261021u);
    const int64_t sizes[] = { 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 8193, 3 * 2048 + 5 };
    CHECK(prefix_blocks(4096) == 1 && prefix_blocks(4097) == 2 && prefix_blocks(8193) == 3);
    for (int64_t n : sizes) one_size(n, rng);
    indices();
    refusals();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("select host ok\n");
    return 0;
}
