// test_mt_jump.cpp — host/mt_jump.hpp against stepping the generator: jump(n) equals n outputs drawn and discarded, jumps compose, a jump
// of 0 leaves the published MT19937 known answers in place, and distances from 2^44 on are an error.  Prints OK and exits 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "../../finmath-lib-cuda-extensions_amd/host/mt_jump.hpp"

using fmhost::MT19937;

static int failures = 0;
static void check(bool ok, const char* what, unsigned long long n) { if (!ok) { std::printf("FAILED: %s (n = %llu)\n", what, n); ++failures; } }

// the next `count` outputs of a and b agree
static bool same_stream(MT19937 a, MT19937 b, int count = 2000) {
    for (int i = 0; i < count; ++i) if (a.next32() != b.next32()) return false;
    return true;
}

int main() {
    const MT19937 seeded((int64_t)31415);
    // jump(n) against stepping: one generator walks on, the distances are visited in increasing order
    unsigned long long dist[] = { 0, 1, 2, (1ull << 5) - 1, (1ull << 5) + 1, 623, 624, 625, (1ull << 10) - 1, (1ull << 10) + 1, 1247, 1248, (1ull << 15) - 1, 1ull << 15,
                                  (1ull << 15) + 1, (1ull << 20) - 1, (1ull << 20) + 1, 10000003ull, (1ull << 24) + 1 };
    MT19937 walker = seeded;
    unsigned long long at = 0;
    for (unsigned long long n : dist) {
        for (; at < n; ++at) walker.next32();
        MT19937 jumped = seeded;
        fmhost::mtJump(jumped, n);
        check(jumped.mti == 624 || n < 624, "state is positioned in front of a regeneration", n);
        check(same_stream(jumped, walker), "jump(n) equals stepping n words", n);
    }
    // from inside a block (mti < 624), and composition jump(a) then jump(b) = jump(a + b)
    {
        MT19937 a = seeded, b = seeded, c = seeded;
        for (int i = 0; i < 100; ++i) a.next32();
        fmhost::mtJump(a, 5000);
        fmhost::mtJump(b, 5100);
        check(same_stream(a, b), "jump from inside a block", 5000);
        fmhost::mtJump(c, 123457); fmhost::mtJump(c, (1ull << 17) + 99);
        MT19937 d = seeded; fmhost::mtJump(d, 123457 + (1ull << 17) + 99);
        check(same_stream(c, d), "jump(a) then jump(b) equals jump(a + b)", 123457);
        // far jumps cannot be stepped: 2^43 + 2^43 − 2^20 … checked by composition: (2^40 + 7) then (2^41 + 11) against the sum
        MT19937 e = seeded, f = seeded;
        fmhost::mtJump(e, (1ull << 40) + 7); fmhost::mtJump(e, (1ull << 41) + 11);
        fmhost::mtJump(f, (1ull << 40) + (1ull << 41) + 18);
        check(same_stream(e, f), "far jumps compose", 1ull << 40);
        MT19937 g = seeded, h = seeded;                      // 2^43 = 2^42 + 2^42: table row 43 against row 42 twice
        fmhost::mtJump(g, 1ull << 43); fmhost::mtJump(h, 1ull << 42); fmhost::mtJump(h, 1ull << 42);
        check(same_stream(g, h), "row 43 equals row 42 applied twice", 1ull << 43);
    }
    // published known answers (mt19937ar.out: init_by_array {0x123, 0x234, 0x345, 0x456}) behind a jump of 0, and behind a jump of 3 outputs
    {
        MT19937 m((int64_t)0);
        const uint32_t key[4] = { 0x123u, 0x234u, 0x345u, 0x456u };
        m.init_by_array(key, 4);
        fmhost::mtJump(m, 0);
        const uint32_t want[5] = { 1067595299u, 955945823u, 477289528u, 4107218783u, 4228976476u };
        for (int i = 0; i < 5; ++i) check(m.next32() == want[i], "mt19937ar known answer after jump(0)", (unsigned long long)i);
        MT19937 k((int64_t)0);
        k.init_by_array(key, 4);
        fmhost::mtJump(k, 3);
        check(k.next32() == want[3] && k.next32() == want[4], "mt19937ar known answer after jump(3)", 3);
    }
    // the limit is an error, not a wrap
    for (unsigned long long n : { 1ull << 44, (1ull << 44) + 1, ~0ull }) {
        MT19937 m = seeded; bool threw = false;
        try { fmhost::mtJump(m, n); } catch (const std::invalid_argument&) { threw = true; }
        check(threw, "distance beyond the table is an error", n);
        check(std::memcmp(m.mt, seeded.mt, sizeof m.mt) == 0, "a refused jump leaves the state alone", n);
    }
    { MT19937 m = seeded; bool threw = false; try { fmhost::mtJump(m, (1ull << 44) - 1); } catch (...) { threw = true; } check(!threw, "2^44 - 1 is allowed", (1ull << 44) - 1); }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
