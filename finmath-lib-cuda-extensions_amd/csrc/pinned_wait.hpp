// pinned_wait.hpp — the one wait for a word of pinned memory that a kernel is about to write.  No HIP and no Engine in it: a stand-alone
// host program can include it (tests/cpp/test_pinned_wait.cpp).
//
// spin_until looks at the word (arrived()), does what its caller wants done between two looks (between(), after every look that failed),
// reads the steady clock every `looks_per_clock` looks and gives up once `budget` has passed: a kernel that takes longer than that is
// waited for the ordinary way, which is the CALLER's business — what follows a timeout is not in here.  It ends with the acquire fence
// (what the device wrote before the word is read after it) and returns whether the word arrived.
//
// The five callers differ in what happens between two looks and in what follows a timeout, on purpose:
//
//   caller                                  between two looks                       clock every   after a timeout                                           engine lock
//   Engine::red_poll (static)               pause                                   1024          returns false                                             NOT held
//   Engine::red_wait, poll flag and         drain_late(late_portion())              64            then red_poll, then wait_for_stream                       held
//     queued releases
//   Engine::slot_wait                       drain if has_late(), else pause         1024          wait_for_stream; still not there: the slot is forgotten   held
//                                                                                                 and it returns false
//   Engine::ticket_take, per slot           as slot_wait                            1024          50 µs naps, hipStreamQuery every 64 naps; NEVER a stream  held
//                                                                                                 synchronise; error if the stream ran dry
//   Engine::pass_wait                       pause only; NO drain_late (the pass     1024          plain hipStreamSynchronize, not wait_for_stream; error    held
//                                           may not rely on a Node*)                              if still not there; pass_dirty_ = false only on success
//
// (the first four: expectations_engine.hpp; the last: side_pass_engine.hpp.  A portion of queued releases takes far longer than a pause,
// hence the clock every 64 looks where every look drains.)
#pragma once

#include <atomic>
#include <chrono>
#include <cstdint>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace fm {

inline void pause() {
#if defined(__x86_64__)
    _mm_pause();
#endif
}

template <class Arrived, class Between>
inline bool spin_until(Arrived arrived, Between between, uint32_t looks_per_clock = 1024,
                       std::chrono::microseconds budget = std::chrono::microseconds(2000)) {
    const auto t0 = std::chrono::steady_clock::now();
    bool there = false;
    for (uint32_t looks = 1; !(there = arrived()); ++looks) {
        between();
        if (looks % looks_per_clock == 0 && std::chrono::steady_clock::now() - t0 > budget) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return there;
}

} // namespace fm
