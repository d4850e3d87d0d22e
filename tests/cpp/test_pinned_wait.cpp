// test_pinned_wait.cpp — spin_until (csrc/pinned_wait.hpp) alone: the one loop behind every wait of the engine for a word of pinned memory.
// A stand-alone host program (no HIP, no engine); tests/test_pinned_wait_cpu.py builds and runs it under AddressSanitizer + UBSan and
// under ThreadSanitizer.
#include "pinned_wait.hpp"

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <thread>

using namespace std::chrono;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    const microseconds budget(2000);
    {   // a word set by a second thread after about 100 µs arrives, and the waiter was between two looks at least once.  (The setter goes
        // only when the waiter has looked once in vain: `between` was called however the threads are scheduled.)
        std::atomic<uint64_t> word{ 0 };
        std::atomic<bool> looked{ false };
        std::thread setter([&] {
            while (!looked.load(std::memory_order_acquire)) std::this_thread::yield();
            std::this_thread::sleep_for(microseconds(100));
            word.store(7, std::memory_order_release);
        });
        uint64_t between = 0;
        // (a budget that cannot run out: the case is about arriving, however slowly the setter's thread is scheduled under a sanitizer)
        const bool arrived = fm::spin_until([&] { return word.load(std::memory_order_relaxed) == 7; },
                                            [&] { ++between; looked.store(true, std::memory_order_release); fm::pause(); }, 1024, seconds(60));
        setter.join();
        CHECK(arrived);
        CHECK(between >= 1);
    }
    {   // a word that is never set: false, after no less than the budget (the upper bound only catches a hang)
        volatile uint64_t word = 0;
        uint64_t looks = 0;
        const auto t0 = steady_clock::now();
        const bool arrived = fm::spin_until([&] { ++looks; return word == 7; }, [] { fm::pause(); }, 1024, budget);
        const auto took = steady_clock::now() - t0;
        CHECK(!arrived);
        CHECK(took >= budget);
        CHECK(took < seconds(30));
        CHECK(looks >= 1024 && looks % 1024 == 0);                // it gives up where it reads the clock, nowhere else
    }
    {   // the defaults are the engine's: the clock every 1024 looks, 2 ms
        volatile uint64_t word = 0;
        uint64_t looks = 0;
        const auto t0 = steady_clock::now();
        CHECK(!fm::spin_until([&] { ++looks; return word == 7; }, [] { fm::pause(); }));
        CHECK(steady_clock::now() - t0 >= milliseconds(2));
        CHECK(looks >= 1024 && looks % 1024 == 0);
    }
    {   // a word already set: true, without a call of `between`
        volatile uint64_t word = 7;
        uint64_t looks = 0, between = 0;
        CHECK(fm::spin_until([&] { ++looks; return word == 7; }, [&] { ++between; }, 1024, budget));
        CHECK(looks == 1 && between == 0);
    }
    // the clock is read every `looks_per_clock` looks: the FIRST call of `between` outlasts the budget, so the wait is over at the first look
    // at the clock — after exactly that many looks, each followed by its `between`.  Nothing here depends on how fast the loop runs.
    for (const uint32_t every : { 64u, 1024u, 1u }) {
        volatile uint64_t word = 0;
        uint64_t looks = 0, between = 0;
        const bool arrived = fm::spin_until([&] { ++looks; return word == 7; },
                                            [&] { if (between++ == 0) std::this_thread::sleep_for(budget + milliseconds(1)); }, every, budget);
        CHECK(!arrived);
        CHECK(looks == every);
        CHECK(between == every);
    }
    {   // … and a word that arrives between two looks at the clock is seen at the next look, not at the next look at the clock
        volatile uint64_t word = 0;
        uint64_t looks = 0;
        CHECK(fm::spin_until([&] { ++looks; return word == 7; }, [&] { if (looks == 10) word = 7; }, 64, budget));
        CHECK(looks == 11);
    }
    if (failures) return 1;
    std::printf("pinned wait ok\n");
    return 0;
}
