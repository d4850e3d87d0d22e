"""The engine's host runtime (csrc/runtime.cpp, abi.cpp, jit.cpp: node pools, intrusive reference counts, replica descriptions, plan caches;
csrc/expectations_engine.hpp: tickets, the pinned arena) under AddressSanitizer + UndefinedBehaviorSanitizer and under ThreadSanitizer, on a TEST-ONLY null device
(tests/nulldev/null_hip.cpp: device memory = host memory, launches compute nothing) — no GPU needed; GPU sanitizers do not exist on this
pool.  tests/nulldev/drive.cpp replays the graph shapes of the GPU tests (replicas in the ten orders of test_gpu_replicas.py, long
chains through segments / rolled / peeled plans, expectations taken along, values given up, tickets out of order, the row-table ring
and the moments arena wrapping at tiny sizes, eight threads, shutdown and re-initialisation) and, in a sweep of its own, a failing
allocation in the middle of a replicated launch of 1100 members and at every allocation of a flush of several replicated groups; `lagging`: a caller whose handles are released late, in bursts, by a
collector thread — the lifetime contract of a JVM (values left unstored, computed from their recipes on demand); `oom`: a device that is
full.  The null device is not a back end and never ships."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NULLDEV = os.path.join(HERE, "nulldev")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-C", NULLDEV, "-j8", "asan", "tsan", "lmm_asan", "lmm_tsan"], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(NULLDEV, "build")


def run(binary, tmp_path, *scenarios, **extra_env):
    env = dict(os.environ, FMHIP_JIT_CACHE_DIR=str(tmp_path / "code_objects"), FMHIP_JIT_PACK_DIR="off", FMHIP_RING_BYTES="16384", FMHIP_ARENA_BYTES="4096",
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    env.update(extra_env)
    return subprocess.run([binary, *scenarios], capture_output=True, text=True, timeout=600, env=env)


def test_host_runtime_is_clean_under_address_and_undefined_behaviour_sanitizers(built, tmp_path):
    r = run(os.path.join(built, "drive_asan"), tmp_path)
    assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-6000:]
    assert r.stdout.count("done") == 16          # eight scenarios, twice (shutdown and re-initialisation in between)
    again = run(os.path.join(built, "drive_asan"), tmp_path)      # once more: the code objects of the first run come from the cache directory
    assert again.returncode == 0 and "Sanitizer" not in again.stderr, again.stderr[-6000:]


def test_host_runtime_is_clean_under_thread_sanitizer(built, tmp_path):
    r = run(os.path.join(built, "drive_tsan"), tmp_path)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stdout[-1500:] + r.stderr[-6000:]
    assert r.stdout.count("done") == 16


def test_a_failing_allocation_inside_a_replicated_launch_leaves_nothing_behind(built, tmp_path):
    """1101 vectors + 1 are allocated before the flush; the 2 x 1101 buffers of the launch follow in two parts of 1024 and 77 members: the
    hook is swept over that stretch.  Every position must leave a process that ends cleanly — no leak, no use after free, no bad status."""
    for at in (1103, 1500, 2125, 2127, 2400, 3150, 3151, 3300, 10**9):
        r = run(os.path.join(built, "drive_asan"), tmp_path, "failure", FMHIP_TEST_FAIL_ALLOC_AT=str(at))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure done" in r.stdout


def test_a_failing_allocation_anywhere_in_a_flush_of_several_replicated_groups_leaves_nothing_behind(built, tmp_path):
    """Scenario `failure_big`: ONE flush of two distinct shapes too long for one launch (segments; 3 and 2 described copies) and the
    two-root graph of `failure` (3 copies).  A counting run says where the flush's pool allocations are; the hook is then put on EVERY
    one of them — which includes the first and the last allocation of each of its launches — and on one beyond the end.  Every position
    must leave a process that ends cleanly: no leak, no use after free, no status but OK / out of memory / a copy marked lost.
    (Before the flush had a guard per group and run_plan dropped half-written cuts, the positions inside the first cutting of either
    long shape — 9 of these 40 — ended in a leak or in a use after free at shutdown.)"""
    import re
    count = run(os.path.join(built, "drive_asan"), tmp_path, "failure_big")
    assert count.returncode == 0 and "Sanitizer" not in count.stderr, count.stdout[-500:] + count.stderr[-6000:]
    before, inside, status = map(int, re.search(r"failure_big: (\d+) allocations before the flush, (\d+) in it, flush status (-?\d+)", count.stdout).groups())
    assert status == 0 and 0 < inside <= 39, "the sweep takes every allocation of the flush, 40 positions at the most"
    for at in range(before + 1, before + inside + 2):
        r = run(os.path.join(built, "drive_asan"), tmp_path, "failure_big", FMHIP_TEST_FAIL_ALLOC_AT=str(at))
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure_big done" in r.stdout
        assert ("flush status 0" in r.stdout) == (at == before + inside + 1), (at, r.stdout[-300:])


@pytest.mark.parametrize("peel_env", [{}, {"FMHIP_PEEL_MAX_WORKGROUPS": "0"}], ids=["peeled", "cut_on_first_use"])
def test_a_failing_allocation_anywhere_in_a_planned_flush_leaves_the_plan_whole(built, tmp_path, peel_env):
    """Scenario `failure_plan`: what `failure_big` (JIT off: segments only) never walks.  One loop-shaped shape too long for one launch —
    the original, two copies that exist as a description, four further members — with its kernels there at once (FMHIP_JIT_SYNC).
    Flush A, the expectation of the original's root, takes the moments of every pending root along: by default as ONE peeled launch of the
    whole group; with FMHIP_PEEL_MAX_WORKGROUPS=0 the plan has no segments yet, run_plan cuts them with the members that have nodes and
    runs the copies from the cuts, the rolled kernel inside.  The hook is put on every allocation of flush A and on one beyond the end of
    the process's (the position right behind flush A is an allocation of flush B).  Flush B — everything released, the same shape recorded
    again, flushed plainly, every root read; done twice, the first pass cuts the shape where A did not get that far — must then be OK
    both times, the second with exactly the launches of the counting run's: a plan that was cut twice, or left half-cut, would run other
    launches.  On the engine before the cuts were committed whole and before a partly run replicated component was closed
    (replicas_after_failure), the second configuration ended in a use after free at every position behind the first segment's launch:
    the copies, still described, ran with what was left of the original and read a value of the ORIGINAL's first segment."""
    import re
    line = re.compile(r"failure_plan: (\d+) allocations before flush A, (\d+) in it, flush A status (-?\d+); flush B status (-?\d+), (\d+) launches")
    count = run(os.path.join(built, "drive_asan"), tmp_path, "failure_plan", **peel_env)
    assert count.returncode == 0 and "Sanitizer" not in count.stderr, count.stdout[-500:] + count.stderr[-6000:]
    before, inside, status_a, status_b, launches_b = map(int, line.search(count.stdout).groups())
    assert status_a == 0 and status_b == 0 and launches_b > 0
    assert 0 < inside <= 80, "the sweep takes every allocation of flush A, 80 positions at the most, and one beyond"
    for at in [*range(before + 1, before + inside + 1), 10**9]:
        r = run(os.path.join(built, "drive_asan"), tmp_path, "failure_plan", FMHIP_TEST_FAIL_ALLOC_AT=str(at), **peel_env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (at, r.stdout[-500:] + r.stderr[-6000:])
        assert "failure_plan done" in r.stdout
        _, _, a, b, launches = map(int, line.search(r.stdout).groups())
        assert a in (0, -3), (at, a)                 # FMHIP_OK or FMHIP_ERR_OUT_OF_MEMORY
        assert b == 0 and launches == launches_b, (at, b, launches, launches_b)


def test_a_full_device(built, tmp_path):
    """The pool's last resort (drop every cached slab, try once more) on the first allocation of a new size class, the out-of-memory
    status, and a fused launch that cannot get its output — on a null device of 800 MB.  Round 5: heap corruption on the real device
    (a reference into the pool's size-class table held across the purge that erases the entry); the native driver under a lagging
    collector and a device that fills up within a few evaluations (collections forced by out-of-memory statuses, retries)."""
    r = run(os.path.join(built, "drive_asan"), tmp_path, "oom", FMNULL_DEVICE_BYTES="800000000", FMHIP_POOL_HEADROOM_BYTES="1000000")
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-500:] + r.stderr[-6000:]
    assert r.stdout.count("oom done") == 2
    for policy in ("0", "1"):
        d = run(os.path.join(built, "lmm_asan"), tmp_path, "--paths", "3000", "--mode", "calibrate", "--max-iterations", "1", "--finmath-like", "--release-lag", "50",
                FMNULL_DEVICE_BYTES="400000000", FMHIP_POOL_HEADROOM_BYTES="20000000", FMHIP_ESCAPE_POLICY=policy, FMHIP_RING_BYTES="1048576", FMHIP_ARENA_BYTES="65536")
        assert d.returncode == 0 and "Sanitizer" not in d.stderr and "runtime error" not in d.stderr, (policy, d.stdout[-500:] + d.stderr[-6000:])
        assert '"collections_forced_by_out_of_memory": 0' not in d.stdout or policy == "1"


@pytest.mark.parametrize("shards", [2, 3])
def test_a_device_list_is_clean_under_both_sanitizer_builds(built, tmp_path, shards):
    """The same scenarios behind fmhip_init_devices (csrc/sharded.cpp: one engine and one worker thread per shard, the caller's calls replayed
    through a single-producer ring per worker, reads and reductions gathered): ASan + UBSan, then ThreadSanitizer."""
    r = run(os.path.join(built, "drive_asan"), tmp_path, FMNULL_DEVICES=str(shards))
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-6000:]
    assert r.stdout.count("done") == 16
    t = run(os.path.join(built, "drive_tsan"), tmp_path, FMNULL_DEVICES=str(shards))
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-1500:] + t.stderr[-6000:]
    assert t.stdout.count("done") == 16


def test_the_expectation_collective_of_a_device_list(built, tmp_path):
    """Expectations wanted ON the devices of a device list: with distinct device indices the front asks RCCL (here: the stand-ins of
    tests/nulldev/null_rccl.cpp, found by dlsym as librccl.so's would be) for a communicator per device and issues ONE all-gather for
    all of them inside ncclGroupStart / ncclGroupEnd, a combine kernel per device follows; with a repeated index the host combines.
    Every device must hold the bits the host-side reduction returns (scenario `collective`), under ASan and TSan, 4 and 8 devices."""
    for env in ({"FMNULL_DEVICES": "4", "FMNULL_DISTINCT": "1"}, {"FMNULL_DEVICES": "8", "FMNULL_DISTINCT": "1"}, {"FMNULL_DEVICES": "3"}):
        r = run(os.path.join(built, "drive_asan"), tmp_path, "collective", "lagging", **env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (env, r.stdout[-500:] + r.stderr[-6000:])
        assert r.stdout.count("done") == 4
    t = run(os.path.join(built, "drive_tsan"), tmp_path, "collective", "lagging", "basic", FMNULL_DEVICES="4", FMNULL_DISTINCT="1")
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-6000:]


def test_the_native_lmm_driver_is_clean_under_both_sanitizer_builds(built, tmp_path):
    """The real workload instead of hand-made scenarios: host/lmm_hip_main.cpp (the LMM calibration driver over the C-ABI) linked against the
    null device — Jacobian batches as replica descriptions, payoff values given up, expectation tickets collected one batch late, rolled and
    peeled plans of the 80-rate simulation, the caller without hints (every method a node, time steps grouped by the engine), a device list
    of two shards, and the path-sharded form whose expectation partials are gathered into a device buffer (RCCL replaced by stand-ins).
    The numbers are meaningless (the null device computes nothing): what is checked is that every one of these runs ends with status 0 and
    nothing for ASan / UBSan / LeakSanitizer, resp. ThreadSanitizer, to report."""
    asan, tsan = os.path.join(built, "lmm_asan"), os.path.join(built, "lmm_tsan")
    base = ["--paths", "3000"]
    cases = [["--mode", "calibrate", "--max-iterations", "1"],
             ["--mode", "evaluate", "--evaluations", "3", "--finmath-like"],
             ["--mode", "calibrate", "--max-iterations", "1", "--devices", "0,0"],
             ["--mode", "calibrate", "--max-iterations", "1", "--world", "1", "--rank", "0", "--nccl-id-file", str(tmp_path / "id"), "--nccl-nonce", "5"],
             # an engine per caller thread (fmhip_set_thread_engines): the Jacobian's columns on four threads, the Brownian increments and the
             # initial curve owned by the first engine and imported by the others, results read and released across threads; two iterations,
             # so that the second pool of threads takes over the engines the first one left behind
             ["--mode", "calibrate", "--max-iterations", "2", "--finmath-like", "--threads", "4"],
             # the caller without hints whose handles die when a collector thread says so (host/random_variable.hpp: ReleaseLag): every 5 ms,
             # and "never, until 2 MB of dead wrappers have piled up"
             ["--mode", "calibrate", "--max-iterations", "1", "--finmath-like", "--release-lag", "5"],
             ["--mode", "evaluate", "--evaluations", "12", "--finmath-like", "--release-lag-bytes", "2000000"]]
    for args in cases:
        r = run(asan, tmp_path, *base, *args, FMHIP_RING_BYTES="1048576", FMHIP_ARENA_BYTES="65536")
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (args, r.stdout[-500:] + r.stderr[-6000:])
        assert '"evaluations"' in r.stdout
        # the swaptions of an exercise date run as merged launches (merged_chains_engine.hpp: merge_families) in every one of these forms
        assert int(r.stdout.split('"merged_launches": ')[1].split(",")[0]) > 0, (args, r.stdout[-800:])
    for args in (cases[0], cases[2], cases[4], cases[5]):
        t = run(tsan, tmp_path, *base, *args, FMHIP_RING_BYTES="1048576", FMHIP_ARENA_BYTES="65536")
        assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, (args, t.stdout[-500:] + t.stderr[-6000:])


def test_a_kernel_another_caller_thread_is_compiling_is_waited_for_and_the_waiter_is_woken(built, tmp_path):
    """Thread engines share one compiler.  With FMHIP_JIT=sync a caller compiles on its own thread; a second thread that asks for the same
    kernel meanwhile waits for it — and must be woken when the first is done (until round 5 only the compiler's worker thread woke such
    waiters: four thread engines that met the merged kernels, which take tens of seconds each, waited for good: the kernel pack recording
    was killed after seven silent minutes).  The null device's hiprtc takes FMNULL_COMPILE_MS per kernel here; no code-object cache."""
    t = run(os.path.join(built, "lmm_tsan"), tmp_path, "--paths", "3000", "--mode", "calibrate", "--max-iterations", "2", "--finmath-like", "--threads", "4",
            FMHIP_JIT="sync", FMHIP_JIT_CACHE_DIR="off", FMNULL_COMPILE_MS="15", FMHIP_RING_BYTES="1048576", FMHIP_ARENA_BYTES="65536")
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-500:] + t.stderr[-4000:]
    assert '"evaluations"' in t.stdout


def test_thread_engines_are_clean_under_both_sanitizer_builds(built, tmp_path):
    """Every scenario again with an engine per caller thread (fmhip_set_thread_engines; csrc/abi.cpp, namespace te): the eight threads of
    `threads` record into engines of their own; `shared` crosses them — a pending vector of the main thread as an operand of six threads
    (exported by its owner, imported as an aliasing leaf), the main thread's program run by the others with mixed operands, tickets begun
    on one thread and ended on another, vectors handed over and released across engines; then shutdown (engines retired) and the same again."""
    r = run(os.path.join(built, "drive_asan"), tmp_path, FMNULL_THREAD_ENGINES="1")
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-1500:] + r.stderr[-6000:]
    assert r.stdout.count("done") == 16
    t = run(os.path.join(built, "drive_tsan"), tmp_path, FMNULL_THREAD_ENGINES="1")
    assert t.returncode == 0 and "ThreadSanitizer" not in t.stderr, t.stdout[-1500:] + t.stderr[-6000:]
    assert t.stdout.count("done") == 16

