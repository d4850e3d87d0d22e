"""The device reduce-by-key on the GPU (include/fmhip.h: fmhip_group_sums; csrc/group_kernel.hip): the device's outputs
EQUAL the host twin's, the definition, as uint32 views, and `ungrouped` is equal — over the sizes, the m and the index families of the CPU
test and n = 4 194 305, the first size with three tiles per chunk, with m = 1000 and m = 2^20; with 0, 1 and 4 value vectors, every mask,
fusion on and off (the inputs pending in the lazy graph when the pass is called); a refusal leaves the pool as it was; the mirror with
FMHIP_DEVICE_GROUP=0 and =1 to the last bit; offspring_counts of a systematic resample's ancestors is np.bincount and sums to n;
conditional_expectation_by_state is the gather of the twin's means; and Merton's series term by term."""
import contextlib
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest

from test_group_cpu import (HOSTILE, MERTON, MERTON_MAX_JUMPS, MERTON_PATHS, MERTON_SEED, MERTON_STEPS, QUIET_NAN, SIZES, bits, check_merton_by_jump_count,
                            families, group_counts_of, values_for)

pytestmark = pytest.mark.gpu


class knob_off:
    def __enter__(self):
        self.prev = os.environ.get("FMHIP_DEVICE_GROUP")
        os.environ["FMHIP_DEVICE_GROUP"] = "0"
    def __exit__(self, *a):
        if self.prev is None: del os.environ["FMHIP_DEVICE_GROUP"]
        else: os.environ["FMHIP_DEVICE_GROUP"] = self.prev


def up(gpu, a):
    return a if isinstance(a, gpu.DeviceVector) else gpu.DeviceVector.from_host(np.ascontiguousarray(a, dtype=np.float32))


def handles(vs):
    return (C.c_int64 * max(len(vs), 1))(*[v.handle for v in vs])


def outputs(mask):
    return bin(mask).count("1")


def device_group(gpu, I, V, m, mask, want_counts=True, want_ungrouped=True):
    """fmhip_group_sums through ctypes on device vectors: (outs as uint32 bits, counts as uint32 bits or None, ungrouped or None)."""
    n_out = len(V) * outputs(mask)
    out = (C.c_int64 * max(n_out, 1))(*([-1] * max(n_out, 1)))
    counts, ungrouped = C.c_int64(-1), C.c_int64(-1)
    gpu._native.check(gpu.lib().fmhip_group_sums(I.handle, m, handles(V) if V else None, len(V), mask, C.byref(counts) if want_counts else None,
                                                 out if V else None, C.byref(ungrouped) if want_ungrouped else None))
    made = [bits(gpu.DeviceVector(int(out[i]), m).to_float32()) for i in range(n_out)]
    return made, (bits(gpu.DeviceVector(counts.value, m).to_float32()) if want_counts else None), (ungrouped.value if want_ungrouped else None)


def twin(gpu, index, values, m, mask):
    """The definition's outputs in the device call's order: vector-major, the mask's bits ascending."""
    what = tuple(w for b, w in ((1, "sum"), (2, "mean"), (4, "variance")) if mask & b)
    outs, counts, ungrouped = gpu.group_sums_host(index, values, m, what=what) if values else gpu.group_sums_host(index, [], m)
    return [bits(o) for row in outs for o in row], bits(counts), ungrouped


def check(gpu, index, values, m, n_values, mask, what, I=None, V=None, want_counts=True, want_ungrouped=True):
    I = up(gpu, index) if I is None else I
    V = ([up(gpu, v) for v in values] if V is None else V)[:n_values]
    want_outs, want_counts_bits, want_ungrouped_value = twin(gpu, index, values[:n_values], m, mask if n_values else 0)
    outs, counts, ungrouped = device_group(gpu, I, V, m, mask if n_values else 0, want_counts, want_ungrouped)
    if want_ungrouped: assert ungrouped == want_ungrouped_value, what
    if want_counts: assert (counts == want_counts_bits).all(), (what, "counts", np.flatnonzero(counts != want_counts_bits)[:5])
    assert len(outs) == len(want_outs)
    for j, (o, w) in enumerate(zip(outs, want_outs)):
        assert (o == w).all(), (what, j, np.flatnonzero(o != w)[:5], o[o != w][:3], w[o != w][:3])


@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_host_twin(gpu, n):
    rng = np.random.default_rng(400 + n)
    values = values_for(n, rng, 4, odd=(n % 2 == 1))
    V = [up(gpu, v) for v in values]
    turn = n
    for m in group_counts_of(n):
        for name, index in families(n, m, rng):
            turn += 1
            if turn % 2: index[rng.random(n) < 0.05] = np.concatenate([HOSTILE, np.float32([m])])[turn % 8]
            I = up(gpu, index)
            check(gpu, index, values, m, 1, 7, (n, m, name, "one vector, every output"), I=I, V=V)
            check(gpu, index, values, m, 0, 0, (n, m, name, "counts only"), I=I, V=V, want_ungrouped=bool(turn % 2))
            check(gpu, index, values, m, 4, 1 + turn % 7, (n, m, name, "four vectors"), I=I, V=V, want_counts=bool(turn % 2))


def test_the_largest_m_with_ungrouped_elements(gpu):
    """m = 2^24: the key of an ungrouped element, m itself, needs 25 bits — a fourth radix pass.  NaN, negative and >= m indices among
    members of group 0, of the last group and of groups in between: the ungrouped run stays behind every group."""
    n, m = 12_289, 1 << 24
    rng = np.random.default_rng(24)
    values = values_for(n, rng, 1)
    index = rng.integers(0, m, n).astype(np.float32)
    index[::5] = 0.0
    index[1::7] = np.float32(m - 1)
    index[2::3] = np.float32([np.nan, -1.0, m, m + 2, -np.inf, 0.5])[np.arange(len(index[2::3])) % 6]
    check(gpu, index, values, m, 1, 1, "m = 2^24 with ungrouped elements")
    check(gpu, index, values, m, 0, 0, "m = 2^24, counts only")
    check(gpu, np.full(n, np.nan, dtype=np.float32), values, m, 1, 2, "m = 2^24, nothing grouped")


@pytest.mark.parametrize("mask", [1, 2, 3, 4, 5, 6, 7])
def test_every_mask(gpu, mask):
    n, m = 12_289, 300
    rng = np.random.default_rng(500 + mask)
    values = values_for(n, rng, 4)
    index = rng.integers(-1, m + 1, n).astype(np.float32)
    for n_values in (1, 4):
        check(gpu, index, values, m, n_values, mask, (mask, n_values), want_counts=(mask % 2 == 0))
    check(gpu, index, values, m, 0, 0, "only the ungrouped count", want_counts=False)


@pytest.mark.parametrize("m", [1000, 1 << 20])
def test_three_tiles_per_chunk(gpu, m):
    """n = 4 194 305: the first size whose chunks have three tiles — the wave totals' two buffers in LDS are written a second time, and the
    open run crosses two tile boundaries inside a chunk.  m = 1000: two radix passes; m = 2^20: three."""
    n = 4_194_305
    rng = np.random.default_rng(600 + m)
    values = values_for(n, rng, 1)
    index = rng.integers(0, m, n).astype(np.float32)
    index[rng.random(n) < 0.01] = np.nan
    check(gpu, index, values, m, 1, 7, ("three tiles per chunk", m))
    if m == 1000: check(gpu, np.zeros(n, dtype=np.float32), values_for(n, rng, 1, odd=False), 1, 1, 1, "one group at three tiles per chunk")


@pytest.mark.parametrize("fusion", [False, True])
@pytest.mark.parametrize("n", [65, 2049, 8193])
def test_pending_inputs(gpu, fusion, n):
    """Fusion on: the index and the values are pending in the lazy graph when the pass is called, and the pass computes them first."""
    rng = np.random.default_rng(700 + n)
    m = 37
    prev = gpu.set_fusion(fusion)
    try:
        base = gpu.RandomVariableHip(0.0, up(gpu, rng.integers(-2, m, n).astype(np.float32)))
        state = gpu.RandomVariableHip(0.0, up(gpu, rng.standard_normal(n).astype(np.float32)))
        for n_values, mask in ((1, 7), (2, 5), (0, 0)):
            index_rv, x_rv, y_rv = base.add(1.0), state.mult(3.0), state.add(base)                # pending with fusion on
            outs, counts, ungrouped = device_group(gpu, index_rv.realizations, [x_rv.realizations, y_rv.realizations][:n_values], m, mask)
            index, values = index_rv.realizations.to_float32(), [x_rv.realizations.to_float32(), y_rv.realizations.to_float32()][:n_values]
            want_outs, want_counts, want_ungrouped = twin(gpu, index, values, m, mask)
            assert ungrouped == want_ungrouped and (counts == want_counts).all()
            for o, w in zip(outs, want_outs): assert (o == w).all()
    finally:
        gpu.set_fusion(prev)


def pool(gpu):
    s = gpu.pool_stats()
    return s.n_live_vectors, s.bytes_in_use


def test_a_refusal_leaves_the_pool_as_it_was(gpu):
    n, m = 8193, 100
    rng = np.random.default_rng(8)
    I, X, longer = up(gpu, rng.integers(0, m, n).astype(np.float32)), up(gpu, rng.standard_normal(n).astype(np.float32)), up(gpu, np.ones(n + 1, dtype=np.float32))
    lib, N = gpu.lib(), gpu._native
    out, counts, u = (C.c_int64 * 12)(*([-7] * 12)), C.c_int64(-7), C.c_int64(-7)
    before = pool(gpu)
    for args, status in (((I.handle, 0, handles([X]), 1, 1), N.ERR_INVALID_ARGUMENT), ((I.handle, (1 << 24) + 1, handles([X]), 1, 1), N.ERR_INVALID_ARGUMENT),
                         ((I.handle, m, handles([X] * 5), 5, 1), N.ERR_INVALID_ARGUMENT), ((I.handle, m, handles([X]), 1, 0), N.ERR_INVALID_ARGUMENT),
                         ((I.handle, m, handles([X]), 1, 8), N.ERR_INVALID_ARGUMENT), ((0, m, handles([X]), 1, 1), N.ERR_INVALID_ARGUMENT),
                         ((I.handle, m, handles([longer]), 1, 1), N.ERR_SIZE_MISMATCH), ((I.handle, m, handles([X, longer]), 2, 7), N.ERR_SIZE_MISMATCH)):
        assert lib.fmhip_group_sums(*args, C.byref(counts), out, C.byref(u)) == status, args
        assert all(int(o) == -7 for o in out) and counts.value == -7 and u.value == -7 and pool(gpu) == before
    assert lib.fmhip_group_sums(I.handle, m, None, 0, 0, None, None, None) == N.ERR_INVALID_ARGUMENT and pool(gpu) == before      # nothing asked for
    made, c, ungrouped = device_group(gpu, I, [X], m, 1)                              # and the same call succeeds; its temporaries went back
    del made, c
    assert ungrouped == 0 and pool(gpu) == before


def test_the_mirror_with_the_knob_off_gives_the_same_bits(gpu):
    n, m = 8193 + 77, 200
    rng = np.random.default_rng(10)
    index, (x, y) = rng.integers(-3, m + 3, n).astype(np.float32), values_for(n, rng, 2)
    rv = lambda a, t: gpu.RandomVariableHip(t, up(gpu, a))
    results = []
    for off in (False, True):
        with (knob_off() if off else contextlib.nullcontext()):
            assert gpu.device_group() == (not off)
            outs, counts, ungrouped = gpu.group_moments(rv(index, 1.0), [rv(x, 2.0), rv(y, 0.5)], m, what=("variance", "sum"), counts=True)
            assert [o.time for row in outs for o in row] == [2.0, 2.0, 1.0, 1.0] and counts.time == 1.0 and counts.realizations.n == m
            (sx,) = gpu.group_sums(rv(index, 1.0), [rv(x, 2.0)], m)
            (my,) = gpu.group_means(rv(index, 1.0), [rv(y, 2.0)], m)
            only_counts, only_ungrouped = gpu.group_counts(rv(index, 0.0), m)
            assert only_ungrouped == ungrouped
            results.append([ungrouped] + [bits(v.realizations.to_float32()).tolist() for v in (outs[0][0], outs[0][1], outs[1][0], outs[1][1], counts, sx, my, only_counts)])
    assert results[0] == results[1]
    want, want_counts, want_ungrouped = gpu.group_sums_host(index, [x, y], m, what=("variance", "sum"))
    assert results[0][0] == want_ungrouped and results[0][1] == bits(want[0][0]).tolist() and results[0][4] == bits(want[1][1]).tolist()
    assert results[0][2] == results[0][6] and results[0][5] == results[0][8] == bits(want_counts).tolist()


def test_offspring_counts_of_a_systematic_resample(gpu):
    n = 8193
    rng = np.random.default_rng(9)
    w = rng.random(n).astype(np.float32); w[rng.random(n) < 0.3] = 0.0
    rv = lambda a: gpu.RandomVariableHip(0.0, up(gpu, a))
    _, ancestors, total = gpu.systematic_resample(rv(w), [rv(w)], 0.375, ancestors=True)
    offspring = gpu.offspring_counts(ancestors, n).realizations.to_float32()
    a = ancestors.realizations.to_float32().astype(np.int64)
    assert (offspring == np.bincount(a, minlength=n).astype(np.float32)).all() and offspring.sum() == n and (offspring[w == 0.0] == 0).all()


def test_conditional_expectation_by_state_is_the_gather_of_the_twins_means(gpu):
    n, m = 12_289, 9
    rng = np.random.default_rng(11)
    state = rng.integers(-1, m + 1, n).astype(np.float32)
    y = (rng.standard_normal(n) + state).astype(np.float32)
    rv = lambda a: gpu.RandomVariableHip(1.5, up(gpu, a))
    got = gpu.conditional_expectation_by_state(rv(state), rv(y), m)
    ((means,),), _, _ = gpu.group_sums_host(state, [y], m, what=("mean",))
    (want,) = gpu.gather_host(state, [means])
    assert got.time == 1.5 and (bits(got.realizations.to_float32()) == bits(want)).all()
    outside = (state < 0) | (state > m - 1)
    assert (bits(want)[outside] == QUIET_NAN).all() and outside.any() and np.isfinite(want[~outside]).all()


def test_merton_series_term_by_term(gpu):
    """merton_call_by_jump_count_mc at 2^18 paths, lam·T = 1, 10 steps: the groups k = 0 … 4 are all compared and further groups where the
    count is at least 1000; per compared group the mean within 4 standard errors of e^{-rT}·Black(F_k, K, σ²T + kδ²) and the share within
    4 binomial standard errors of the Poisson probability (about a dozen comparisons at once).  The seed was fixed after
    tests/test_group_cpu.py::test_the_merton_comparison_holds_for_the_definition_alone passed with it on the CPU — the increments of
    fmhip_increments_host, the driver's arithmetic in numpy and the twin: the definition alone passes."""
    mc = import_module("finmath-lib-cuda-extensions_amd.montecarlo")
    td = gpu.TimeDiscretization(0.0, MERTON_STEPS, MERTON["maturity"] / MERTON_STEPS)
    prev = gpu.set_fusion(True)
    try:
        inc = gpu.merton_increments(td, MERTON_PATHS, MERTON_SEED, MERTON["jump_intensity"])
        result = mc.merton_call_by_jump_count_mc(inc, max_jumps=MERTON_MAX_JUMPS, **MERTON)
        assert check_merton_by_jump_count(result, MERTON_PATHS) >= 5
        assert result["ungrouped"] == 0 and len(result["mean"]) == MERTON_MAX_JUMPS + 1
        with knob_off():
            host = mc.merton_call_by_jump_count_mc(inc, max_jumps=MERTON_MAX_JUMPS, **MERTON)
        assert host["count"] == result["count"] and host["ungrouped"] == result["ungrouped"]
        assert [np.float32(v).view(np.uint32) for v in host["mean"]] == [np.float32(v).view(np.uint32) for v in result["mean"]]
    finally:
        gpu.set_fusion(prev)
