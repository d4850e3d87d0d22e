"""The rolled, peeled and merged loop kernels (loop_engine.hpp: detect_loop, plan_peel; merged_chains_engine.hpp: merge_families; jit.cpp: jit_generate_rolled_source,
jit_generate_merged_source) over the catalogue of tests/loop_shapes.py: every operand form and limit of the generator, bit for bit
against the oracle, in the three modes the other loop tests use — the segmented launches of the interpreter tier, the run that meets the
shape with the specialised tier on, and the run after it — with the engine's own counter as the proof of which kernel ran, and the
descriptions the engine recorded as the proof that a shape reached the path it was written for."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import arith_cases as ac
import loop_shapes as ls
from conftest import assert_bits_equal
from test_gpu_merged_chains import moments_tuple
from test_gpu_parity_ops import assert_libm_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 6149                                  # three tiles of 2048 and a ragged one at 8 elements per lane, six tiles at 4
EDGE_SIZES = [1, 2047, 2048, 2049]
PLANTED_VALUES = ac.f32([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42])
POSITIONS = ("every_slot", "one_per_wave", "last_element")
MODES = ("segments", "discovery", "rolled")

_cache = {}


def case(oracle, shape, n, planted=None, seed=0):
    """(data, the oracle's kept vectors) of a shape at a size, computed once and shared; `planted` = a name of ac.placements."""
    key = (shape.name, n, planted, seed)
    if key not in _cache:
        d = shape.data(np.random.default_rng([n, seed, zlib.crc32(shape.name.encode())]), n)
        if planted:
            at = ac.placements(n)[planted]
            k = 0
            for name in shape.plantable:
                targets = [0, len(d[name]) // 2, len(d[name]) - 1] if isinstance(d[name], list) else [None]
                for t in targets:                       # the first, a middle and the last iteration's input; a loop-invariant vector as it is
                    values = np.roll(PLANTED_VALUES, k)     # (a single position meets another value in every vector)
                    if t is None: d[name] = ac.plant(d[name], at, values)
                    else: d[name][t] = ac.plant(d[name][t], at, values)
                    k += 1
        with np.errstate(all="ignore"):
            want = shape.oracle(oracle, d)
        for w in want.values():
            w.setflags(write=False)
        _cache[key] = (d, want)
    return _cache[key]


def poison(gpu, n):
    """Every buffer of n elements that the pool holds back for reuse is overwritten with NaN.  The modes (and the tests) run the same
    data one after the other, and a vector is computed into whatever buffer the pool hands out: without this a store that a kernel never
    makes would leave the bits an earlier run wrote there — the right ones."""
    import gc
    gc.collect()
    count = min(gpu.pool_stats().bytes_cached // (4 * n) + 8, 4096)
    junk = [gpu.DeviceVector.filled(n, float("nan")) for _ in range(count)]
    gpu.flush()
    del junk


def run_modes(gpu, record, n, math=None):
    """`record()` → {name: DeviceVector} under a hold, flushed, in the three modes: ({mode: {name: array}}, {mode: growth of the counters})."""
    results, grown = {}, {}
    prev_fusion = gpu.set_fusion(True)
    prev_math = gpu.set_math_mode(math) if math is not None else None
    try:
        for mode in MODES:
            prev_jit = gpu.set_jit(gpu.JIT_OFF if mode == "segments" else gpu.JIT_SYNC)
            poison(gpu, n)
            if mode == "segments":
                gpu.purge()                       # forget plans made with another tier setting
            try:
                with gpu.holding():
                    kept = record()
                before = gpu.engine_stats()
                gpu.flush()
                after = gpu.engine_stats()
                grown[mode] = {k: after[k] - before[k] for k in ("rolled_launches", "kernel_launches")}
                results[mode] = {k: v.to_float32() for k, v in kept.items()}
                del kept
            finally:
                gpu.set_jit(prev_jit)
    finally:
        if prev_math is not None: gpu.set_math_mode(prev_math)
        gpu.set_fusion(prev_fusion)
    return results, grown


def assert_all_bits(results, want, what):
    for mode, res in results.items():
        assert res.keys() == want.keys()
        for name in want:
            msg = ac.first_difference(res[name], want[name], f"{what}, {mode}: {name}")
            assert msg is None, msg


def assert_rolled(shape, grown):
    if shape.expect is None:
        return
    assert grown["segments"]["rolled_launches"] == 0, grown
    assert grown["rolled"]["rolled_launches"] >= 1, f"{shape.name}: no launch of a loop kernel in the third mode: {grown}"


@pytest.mark.parametrize("shape", ls.EXACT, ids=repr)
def test_shape_equals_the_oracle_in_every_mode(gpu, oracle, shape):
    """What happened to the shapes whose rolling is the engine's business (MI355X, this commit; `rolled` = loop launches of the third mode):
    aliased_two_iterations 0 (detect_loop: "input used by more than one iteration" — the whole component stays on its segments),
    aliased_both_slots 1 (the 30 iterations behind iteration 7 roll, plain kernel), aliased_global_and_input 1 (the 21 iterations behind
    iteration 17), carried_13 / inputs_13 / scalars_49 / period_129 / period12_one_fewer 0."""
    d, want = case(oracle, shape, N)
    dev = ls.to_device(gpu, d)
    results, grown = run_modes(gpu, lambda: shape.device(dev), N)
    print(shape.name, grown)
    assert_all_bits(results, want, shape.name)
    assert_rolled(shape, grown)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_two_carried_at_the_tile_edges(gpu, oracle, n):
    d, want = case(oracle, ls.TWO_CARRIED, n)
    dev = ls.to_device(gpu, d)
    results, grown = run_modes(gpu, lambda: ls.TWO_CARRIED.device(dev), n)
    assert_all_bits(results, want, f"two_carried, n = {n}")
    assert_rolled(ls.TWO_CARRIED, grown)


def test_three_members_of_one_launch(gpu, oracle):
    """many_io three times under one hold — the same loop-invariant vectors, inputs and scalars of its own each: rows of ONE loop launch."""
    shape = ls.MANY_IO
    cases = [case(oracle, shape, N, seed=m) for m in range(3)]
    data = []
    for m, (d, _) in enumerate(cases):
        d = dict(d, g0=cases[0][0]["g0"], g1=cases[0][0]["g1"], s=[v + 0.125 * m for v in d["s"]])
        data.append(d)
    with np.errstate(all="ignore"):
        want = {f"{m}.{k}": v for m, d in enumerate(data) for k, v in shape.oracle(oracle, d).items()}
    shared = ls.to_device(gpu, {"g0": data[0]["g0"], "g1": data[0]["g1"]})
    devs = [dict(ls.to_device(gpu, d), **shared) for d in data]
    results, grown = run_modes(gpu, lambda: {f"{m}.{k}": v for m, dev in enumerate(devs) for k, v in shape.device(dev).items()}, N)
    assert_all_bits(results, want, "three members")
    assert grown["segments"]["rolled_launches"] == 0 and grown["rolled"]["rolled_launches"] == 1, grown


@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("shape", ls.PLANTED, ids=repr)
def test_planted_values(gpu, oracle, shape, position):
    """NaN, ±inf, ±0 and a denormal in the inputs of the first, a middle and the last iteration and in the loop-invariant vector."""
    d, want = case(oracle, shape, N, planted=position)
    for name, w in want.items():                  # a shape that turns all-NaN checks nothing
        assert np.isfinite(w).mean() > 0.5, f"{shape.name}, {position}: {name} holds {np.isfinite(w).mean():.0%} finite values"
    assert any(not np.isfinite(w).all() for w in want.values()), "nothing planted arrived"
    dev = ls.to_device(gpu, d)
    results, grown = run_modes(gpu, lambda: shape.device(dev), N)
    assert_all_bits(results, want, f"{shape.name}, planted at {position}")
    assert_rolled(shape, grown)


# ---------------------------------------------------------------------------------------------- library mathematics
def eager(gpu, shape, dev, math=None):
    """The eager device run: fusion off, one launch per method (the reference of test_gpu_merged_chains.py)."""
    prev_fusion = gpu.set_fusion(False)
    prev_math = gpu.set_math_mode(math) if math is not None else None
    try:
        return {k: v.to_float32() for k, v in shape.device(dev).items()}
    finally:
        if prev_math is not None: gpu.set_math_mode(prev_math)
        gpu.set_fusion(prev_fusion)


@pytest.mark.parametrize("shape,n", [(ls.LIBRARY_MATH, n) for n in [N] + EDGE_SIZES] + [(ls.PEELED_LIBRARY, N)], ids=repr)
def test_library_shapes_equal_the_eager_run(gpu, oracle, shape, n):
    """exp / log / pow / sin / cos are evaluated in fp64 and narrowed once on both sides: the eager run against the oracle within the
    contract of test_gpu_parity_ops.py, every mode against the eager run bit for bit (the same device functions in the same order)."""
    d, want = case(oracle, shape, n)
    dev = ls.to_device(gpu, d)
    reference = eager(gpu, shape, dev)
    for name in want:
        assert_libm_close(reference[name], want[name], f"{shape.name}: eager {name} against the oracle")
    results, grown = run_modes(gpu, lambda: shape.device(dev), n)
    assert_all_bits(results, reference, f"{shape.name}, n = {n}")
    assert_rolled(shape, grown)


def test_library_math_fast_modes_agree(gpu, oracle):
    """MATH_FAST has no oracle: the three modes give the same bits (and, with hardware exp / log, not the exact mode's)."""
    d, _ = case(oracle, ls.LIBRARY_MATH, N)
    dev = ls.to_device(gpu, d)
    results, grown = run_modes(gpu, lambda: ls.LIBRARY_MATH.device(dev), N, math=gpu.MATH_FAST)
    assert_all_bits(results, results["segments"], "library_math, MATH_FAST")
    assert_rolled(ls.LIBRARY_MATH, grown)
    assert np.isfinite(results["rolled"][f"c{ls.ITERATIONS - 1}"]).all()


def test_moments_of_a_pending_peeled_library_chain(gpu, oracle):
    """The peeled kernel at 4 elements per lane takes no moments itself (plan_peel: the variant exists at 8 only): `.moments()` on the
    pending chain must run the chain and then the stand-alone reduction — whose bits these are, shifted or not."""
    shape = ls.PEELED_LIBRARY
    d, _ = case(oracle, shape, N)
    dev = ls.to_device(gpu, d)
    reference = eager(gpu, shape, dev)["value"]
    prev_fusion, prev_jit = gpu.set_fusion(True), gpu.set_jit(gpu.JIT_SYNC)
    try:
        def chain():
            with gpu.holding():
                return shape.device(dev)["value"]
        chain().to_float32()                              # discovery
        plain = chain()
        gpu.flush()
        want = plain.moments()                            # the stand-alone reduction of the materialised vector
        mean = want.sum / N
        for shift, ref in ((0.0, want), (mean, plain.moments(shift=mean))):
            poison(gpu, N)
            c = chain()
            before = gpu.engine_stats()["rolled_launches"]
            got = c.moments(shift=shift)                  # asked while pending
            assert gpu.engine_stats()["rolled_launches"] == before + 1, "the pending chain ran as its peeled kernel"
            assert np.array(moments_tuple(got)).tobytes() == np.array(moments_tuple(ref)).tobytes(), (shift, moments_tuple(got), moments_tuple(ref))
            assert_bits_equal(c.to_float32(), reference, "the value behind the moments")
    finally:
        gpu.set_jit(prev_jit)
        gpu.set_fusion(prev_fusion)


# ---------------------------------------------------------------------------------------------- merged families
def run_family(gpu, fam, L, num, rounds=3):
    """test_gpu_merged_chains.py's procedure: everything recorded under a soft hold, the first `.moments()` runs all that is pending.
    Per round: (moments, values, growth of the counters)."""
    out = []
    prev_fusion, prev_jit, prev_hold = gpu.set_fusion(True), gpu.set_jit(gpu.JIT_SYNC), gpu.fusion_hold(2)
    try:
        poison(gpu, L[0].n)
        gpu.purge()
        for _ in range(rounds):
            poison(gpu, L[0].n)
            values = [ls.family_chain(kind, L, num, periods, rate) for kind, periods, rate in fam.products]
            before = gpu.engine_stats()
            moments = [moments_tuple(v.moments()) for v in values]
            after = gpu.engine_stats()
            out.append((moments, [v.to_float32() for v in values], {k: after[k] - before[k] for k in ("merged_launches", "merged_chains", "rolled_launches")}))
            del values
    finally:
        gpu.fusion_hold(prev_hold)
        gpu.set_jit(prev_jit)
        gpu.set_fusion(prev_fusion)
    return out


def family_data(oracle, fam, n):
    rng = np.random.default_rng([n, zlib.crc32(fam.name.encode())])
    return [ls.uniform(rng, n, fam.lo, fam.hi) for _ in range(fam.vectors)], ls.uniform(rng, n, 0.9, 1.4)


@pytest.mark.parametrize("fam", ls.FAMILIES, ids=repr)
def test_merged_family(gpu, oracle, fam):
    """Every product reads the date's first `periods` vectors from the last one back to L[0]: a suffix of the longest one's sequence.  Values: the oracle's bits; moments: those of the
    stand-alone reduction of the eager value; which products were chains of merged launches: the catalogue says, per family.  Of seventeen tenors SIXTEEN are:
    merge_families closes a family at 16 chains and opens the next one, which needs two chains to be a family (`fam.chain.size() >= 2`) —
    the seventeenth, alone behind the split, runs as a launch of its own."""
    L_h, num_h = family_data(oracle, fam, N)
    want = [ls.family_chain_oracle(oracle, kind, L_h, num_h, periods, rate) for kind, periods, rate in fam.products]
    prev_fusion = gpu.set_fusion(False)
    try:
        L, num = [gpu.DeviceVector.from_host(x) for x in L_h], gpu.DeviceVector.from_host(num_h)
        eager_values = [ls.family_chain(kind, L, num, periods, rate) for kind, periods, rate in fam.products]
        for i, v in enumerate(eager_values):
            assert_bits_equal(v.to_float32(), want[i], f"eager product {i} against the oracle")
        want_moments = [moments_tuple(v.moments()) for v in eager_values]
        del eager_values
    finally:
        gpu.set_fusion(prev_fusion)
    for r, (moments, values, grown) in enumerate(run_family(gpu, fam, L, num)):
        print(fam.name, r, grown)
        for i in range(len(fam.products)):
            assert moments[i] == want_moments[i], f"round {r}: moments of product {i} {fam.products[i]}: {moments[i]} vs {want_moments[i]}"
            assert_bits_equal(values[i], want[i], f"round {r}: product {i} {fam.products[i]}")
        if r >= 1:                                # round 0 plans the shapes, from round 1 on the families are found
            assert grown["merged_launches"] == 1, grown
            assert grown["merged_chains"] == fam.merged, grown
            assert grown["rolled_launches"] >= grown["merged_launches"], grown


# ---------------------------------------------------------------------------------------------- the descriptions the engine recorded
_CHILD = r'''
import importlib, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import loop_shapes as ls
import oracle
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
from test_gpu_loop_shapes import N, family_data, run_family
fm.init(0)
fm.set_fusion(True)

def mark(name):
    with open(%(record)r, "a") as f:
        f.write("# shape " + name + "\n")

for shape in ls.ROLLING:
    mark(shape.name)
    dev = ls.to_device(fm, shape.data(np.random.default_rng(1), N))
    with fm.holding():
        kept = shape.device(dev)
    fm.flush()
    for v in kept.values():
        v.to_float32()
    del kept
for fam in ls.FAMILIES:
    mark(fam.name)
    L_h, num_h = family_data(oracle, fam, N)
    run_family(fm, fam, [fm.DeviceVector.from_host(x) for x in L_h], fm.DeviceVector.from_host(num_h), rounds=2)
print("DONE")
fm.shutdown()
'''


def test_recorded_descriptions(tmp_path):
    """A fresh process (FMHIP_JIT_RECORD is read once) runs the catalogue with FMHIP_JIT=sync; every shape meant to roll left a description
    with the counts stated next to it — globals, inputs, carried, final and stored positions, elements per lane, peeled or not — every
    family a merged kernel of its size, and the kernel-pack tool reads every line back unchanged."""
    record = tmp_path / "recorded.txt"
    script = tmp_path / "catalogue.py"
    script.write_text(_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests"), "record": str(record)})
    env = dict(os.environ, FMHIP_JIT="sync", FMHIP_JIT_RECORD=str(record))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "DONE" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    by_shape, name = {}, None
    for line in record.read_text().splitlines():
        if line.startswith("# shape "):
            name = line[8:]
            by_shape[name] = []
        else:
            desc = ls.parse_rolled(line)
            if desc is not None:
                by_shape[name].append(desc)
    for shape in ls.ROLLING:
        found = by_shape[shape.name]
        assert any(ls.matches(desc, shape.expect) for desc in found), \
            f"{shape.name}: meant {shape.expect}, recorded {[{k: desc[k] for k in shape.expect} for desc in found]}"
    # what the shapes were written for beyond the counts
    peeled = lambda name: [desc for desc in by_shape[name] if desc["peel"]]
    assert all(desc["log"] == 1 for desc in by_shape["library_math"]), "the log table inside a loop kernel"
    assert all(not desc["reduce"] for desc in by_shape["peeled_library_moments"]), "no moments at 4 elements per lane"
    long_head = peeled("long_head_reload")[0]
    assert len(long_head["pre"]) > 6 and len(long_head["preout"]) == 1 and len(long_head["postout"]) == 2, long_head
    assert any(op.split(":")[1:4].count("p" + long_head["preout"][0]) for op in long_head["post"]), "the tail reads the stored head value back"
    plain = [desc for desc in by_shape["final_not_carried"] if not desc["peel"]][0]
    assert set(plain["final_pos"]) - set(plain["carried_pos"]) and not peeled("final_not_carried"), "a final value that is not carried, stored by a plain kernel"
    for shape, slots in ((ls.OPERAND_SLOTS_3, (1, 2, 3)), (ls.OPERAND_SLOTS_2, (1, 2))):          # the carried register itself in every operand position
        body = [op.split(":") for op in by_shape[shape.name][0]["body"]]
        for slot in slots:
            assert sum(op[slot] == "c0" for op in body) >= 4, (shape.name, slot)
    assert all(f == "0" for descs in by_shape.values() for desc in descs for f in desc["finalstore"]), "the engine asked a peeled kernel to store a final value"
    for fam in ls.FAMILIES:
        sizes = sorted(desc["chains"] for desc in by_shape[fam.name] if desc["chains"])
        assert sizes == sorted(fam.kernels), (fam.name, sizes)
    tool = os.path.join(ROOT, "finmath-lib-cuda-extensions_amd", "build", "jit_pack_tool")
    # where the generated kernels store through their row: every value the description says, into the word of the row that is its
    for name, descs in by_shape.items():
        for desc in descs:
            if desc["chains"]:
                continue
            source = subprocess.run([tool, "--source", str(record), desc["line"]], capture_output=True, text=True, timeout=120).stdout
            stores = set(re.findall(r"reinterpret_cast<gfloat4\*>\(rowp\[(\d+)\]\); [^;]*; [^;]*; [^;]*\{ const f32x4 \w+ = \{ (\w+)\[4 \* t\]", source))
            assert source and stores == ls.expected_row_stores(desc), (name, desc["line"], sorted(stores), sorted(ls.expected_row_stores(desc)))
    check = subprocess.run([tool, "--check", str(record)], capture_output=True, text=True, timeout=120)
    assert check.returncode == 0 and " 0 round-trip differences" in check.stdout, check.stdout[-2000:] + check.stderr[-2000:]
