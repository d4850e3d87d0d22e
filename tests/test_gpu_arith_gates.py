"""The range-gated arithmetic of csrc/fm_device_math.hpp where its gates are: the short division chain (ueval_div_all /
ueval_div_prepared: in-range chain, wave-uniform fallback to the full expansion for operands outside [2^-48, 2^48)), the fast square
root (sqrt_all: [2^-63, 2^63)), the special exponents of pow_all and the thresholds of exp — every operand class of
tests/arith_cases.py through every dividing micro-op in both operand forms, on every way the product executes them (eager calls,
explicit programs on both tiers, lazily fused chains, rolled / peeled loop kernels, merged chains with a shared denominator), against
references that do not go through oracle/ (numpy fp64 narrowed once; mpmath), and a strided sweep over all fp32 bit patterns against
the oracle (the in-suite descendant of benchmarks/exhaustive_unary.py)."""
import contextlib
import functools

import numpy as np
import pytest

import arith_cases as ac

pytestmark = pytest.mark.gpu



def dv(gpu, arr):
    return gpu.DeviceVector.from_host(ac.f32(arr))


@contextlib.contextmanager
def modes(gpu, jit=None, fusion=None, math=None):
    prev_jit = gpu.set_jit(jit) if jit is not None else None
    prev_fusion = gpu.set_fusion(fusion) if fusion is not None else None
    prev_math = gpu.set_math_mode(math) if math is not None else None
    try:
        yield
    finally:
        if prev_math is not None: gpu.set_math_mode(prev_math)
        if prev_fusion is not None: gpu.set_fusion(prev_fusion)
        if prev_jit is not None: gpu.set_jit(prev_jit)


def check(msg):
    assert msg is None, msg


# name -> (public opcode, vector operands, operand that sits in the accumulator, has a scalar, reference(a, b, c, s))
FORMS = {
    "DIV": ("DIV", 2, 0, False, lambda a, b, c, s: ac.ref_div(a, b)),
    "VID": ("DIV", 2, 1, False, lambda a, b, c, s: ac.ref_div(a, b)),                     # the denominator in the accumulator
    "DISCOUNT_A": ("DISCOUNT", 2, 0, True, lambda a, b, c, s: ac.ref_discount(a, b, s)),
    "DISCOUNT_B": ("DISCOUNT", 2, 1, True, lambda a, b, c, s: ac.ref_discount(a, b, s)),   # the rate in the accumulator
    "ADDRATIO_A": ("ADDRATIO", 3, 0, False, lambda a, b, c, s: ac.ref_addratio(a, b, c)),
    "SUBRATIO_A": ("SUBRATIO", 3, 0, False, lambda a, b, c, s: ac.ref_subratio(a, b, c)),
    "INVERT": ("INVERT", 1, 0, False, lambda a, b, c, s: ac.ref_div(np.ones_like(a), a)),
    "SQRT": ("SQRT", 1, 0, False, lambda a, b, c, s: ac.ref_sqrt(a)),
    "DIV_S": ("DIV_S", 1, 0, True, lambda a, b, c, s: ac.ref_div(a, np.full_like(a, np.float32(s)))),
    "VID_S": ("VID_S", 1, 0, True, lambda a, b, c, s: ac.ref_div(np.full_like(a, np.float32(s)), a)),
}
BINARY = ("DIV", "VID", "DISCOUNT_A", "DISCOUNT_B", "ADDRATIO_A", "SUBRATIO_A")
UNARY = ("INVERT", "SQRT", "DIV_S", "VID_S")
SCALAR_OF = {"DISCOUNT_A": 0.5, "DISCOUNT_B": 0.5, "DIV_S": 3.0, "VID_S": 3.0}


def operands_of(form, a, b):
    """(a, b, c) as the form's reference takes them, from a numerator-like and a denominator-like vector."""
    if form in ("ADDRATIO_A", "SUBRATIO_A"):
        return np.roll(a, 4321), a, b                      # acc + a / b
    if form in ("DISCOUNT_A", "DISCOUNT_B"):
        return a, ac._add(ac._mul(b, 2.0), -2.0 * np.ones_like(b)), b        # a / (1 + r·0.5) with r = 2b - 2: the denominator is (nearly) b
    return a, b, b


def build(gpu, form, s):
    """The form as an explicit program: the operand meant for the accumulator comes out of an exact multiplication by one."""
    op, nvec, acc, has_s, _ = FORMS[form]
    p = gpu.Program(3)
    args = list(range(nvec))
    args[acc] = p.op("MULT_S", acc, s=1.0)
    w = p.op(op, *args, s=s) if has_s else p.op(op, *args)
    p.output(w)
    p.reduce(w)
    return p.compile()


def run_both_tiers(gpu, form, s, rows):
    """rows: list of (label, a, b, c) host vectors.  Runs each row on the interpreter and on the specialised kernel; returns
    {jit mode: [(output, moments)]} after asserting the tier that ran."""
    res = {}
    for jit, tier in ((gpu.JIT_OFF, 0), (gpu.JIT_SYNC, 1)):
        with modes(gpu, jit=jit):
            p = build(gpu, form, s)
            assert p.tier()[0] == tier, (form, jit, p.tier())
            out = []
            for label, a, b, c in rows:
                outs, m = p.run([[dv(gpu, a), dv(gpu, b), dv(gpu, c)]])
                out.append((outs[0][0].to_float32(), m))
            assert p.tier()[0] == tier
            res[jit] = out
    return res


def planted_rows(form):
    """In-range vectors of many sizes with out-of-range elements planted into one operand at a time (tests/arith_cases.py: placements)."""
    outside = ac.OUTSIDE_SQRT if form == "SQRT" else ac.OUTSIDE_DIV
    rows = []
    for n in [k for k in ac.RAGGED_SIZES if k > 0] + ac.LARGE_SIZES:
        base = [ac.in_range_vector(n, 10 * n + k) for k in range(3)]
        if form == "SQRT":
            base[0] = np.abs(base[0])
        big = n >= 100000
        for k, (name, idx) in enumerate(ac.placements(n).items()):
            if not big and name not in ("last_element", "one_per_wave", "exactly_one"):
                continue
            for operand in ((0, 1) if big and form in BINARY else (k % 2,)):
                vecs = list(base)
                if form in ("DISCOUNT_A", "DISCOUNT_B") and operand == 1:
                    vecs[1] = ac.plant(base[1], idx, ac.f32([-2.0, 2.0 ** 50, -2.0 ** 49, np.inf, np.nan]))       # 1 + r/2 = 0, 2^49, -2^48, inf, NaN
                elif form in ("ADDRATIO_A", "SUBRATIO_A"):
                    vecs[1 + operand] = ac.plant(base[1 + operand], idx, outside)
                else:
                    vecs[operand if form in BINARY else 0] = ac.plant(base[operand if form in BINARY else 0], idx, outside)
                rows.append((f"n={n}, {name}, planted into operand {operand}", *vecs))
    return rows


def reference(form, s, a, b, c):
    return FORMS[form][4](a, b, c, s)


def shifted(idx, k, n):
    """idx + k, without what falls off the end of a vector of n elements."""
    return (idx + k)[idx + k < n]


@functools.lru_cache(maxsize=None)
def class_rows(kind):
    if kind == "binary":
        (a, b), names = ac.concatenated(ac.binary_classes())
        return a, b, names
    (x,), names = ac.concatenated(ac.unary_classes())
    return x, x, names


# ------------------------------------------------------------------------------------------------ 1. eager calls
def test_eager_calls_on_every_class(gpu):
    a, b, names = class_rows("binary")
    x, _, unames = class_rows("unary")
    with modes(gpu, fusion=False):
        va, vb = dv(gpu, a), dv(gpu, b)
        check(ac.first_difference_by_class(va.v2s0("DIV", vb).to_float32(), ac.ref_div(a, b), names, "eager DIV"))
        c = np.roll(a, 4321)
        vc = dv(gpu, c)
        check(ac.first_difference_by_class(vc.v3s0("ADDRATIO", va, vb).to_float32(), ac.ref_addratio(c, a, b), names, "eager ADDRATIO"))
        check(ac.first_difference_by_class(vc.v3s0("SUBRATIO", va, vb).to_float32(), ac.ref_subratio(c, a, b), names, "eager SUBRATIO"))
        vx = dv(gpu, x)
        num = np.roll(x, 999)
        vnum = dv(gpu, num)
        check(ac.first_difference_by_class(vx.v1s0("SQRT").to_float32(), ac.ref_sqrt(x), unames, "eager SQRT"))
        check(ac.first_difference_by_class(vx.v1s0("INVERT").to_float32(), ac.ref_div(np.ones_like(x), x), unames, "eager INVERT"))
        for s in (0.5, -1.0, 2.0 ** 24, 2.0 ** 90, np.inf):
            check(ac.first_difference_by_class(vnum.v2s1("DISCOUNT", vx, s).to_float32(), ac.ref_discount(num, x, s), unames, f"eager DISCOUNT {s!r}"))
        for s in ac.SCALARS:
            sv = np.full_like(x, np.float32(s))
            check(ac.first_difference_by_class(vx.v1s1("DIV_S", s).to_float32(), ac.ref_div(x, sv), unames, f"eager DIV_S {s!r}"))
            check(ac.first_difference_by_class(vx.v1s1("VID_S", s).to_float32(), ac.ref_div(sv, x), unames, f"eager VID_S {s!r}"))
        for name, r, s in ac.discount_denominators():
            n = np.resize(ac.HARMLESS, r.size)
            check(ac.first_difference(dv(gpu, n).v2s1("DISCOUNT", dv(gpu, r), s).to_float32(), ac.ref_discount(n, r, s), f"eager DISCOUNT, {name}"))


# ------------------------------------------------------------------------------------------------ 2. explicit programs, both tiers
@pytest.mark.parametrize("form", BINARY + UNARY)
def test_program_tiers_on_every_class_and_placement(gpu, form):
    s = SCALAR_OF.get(form, 0.0)
    a, b, names = class_rows("binary" if form in BINARY else "unary")
    rows = [("classes", *operands_of(form, a, b))] + planted_rows(form)
    res = run_both_tiers(gpu, form, s, rows)
    compared = 0
    for k, (label, ra, rb, rc) in enumerate(rows):
        (o0, m0), (o1, m1) = res[gpu.JIT_OFF][k], res[gpu.JIT_SYNC][k]
        want = reference(form, s, ra, rb, rc)
        for tier, got in (("interpreter", o0), ("specialised", o1)):
            if k == 0:
                check(ac.first_difference_by_class(got, want, names, f"{form}, {tier}"))
            else:
                check(ac.first_difference(got, want, f"{form}, {tier}, {label}"))
        assert np.array_equal(m0, m1, equal_nan=True), f"{form}, {label}: fused moments of the two tiers differ: {m0} vs {m1}"
        compared += want.size
    assert compared > 1_000_000


def test_discount_gate_looks_at_the_denominator(gpu):
    """1 + r·s leaves the range (zero, 2^48, infinite, NaN) while the rate r is an ordinary number: both operand forms, both tiers."""
    for name, r, s in ac.discount_denominators():
        n = 4099
        rate = ac.plant(ac.in_range_vector(n, 5, 0.001, 0.01), ac.placements(n)["one_per_wave"], r)
        if "nan" in name or "infinite" in name or "tiny" in name:
            rate = np.resize(r, n)                       # any rate times this scalar leaves the range
        num = ac.in_range_vector(n, 6)
        want = ac.ref_discount(num, rate, s)
        for form in ("DISCOUNT_A", "DISCOUNT_B"):
            res = run_both_tiers(gpu, form, s, [(name, num, rate, rate)])
            for jit, out in res.items():
                check(ac.first_difference(out[0][0], want, f"{form}, jit mode {jit}, {name}"))


# ------------------------------------------------------------------------------------------------ 3. a lazily fused chain
def test_division_inside_a_lazily_fused_chain(gpu):
    a, b, names = class_rows("binary")
    rows = [("classes", a, b)]
    n = ac.LARGE_SIZES[0]
    base = ac.in_range_vector(n, 1), ac.in_range_vector(n, 2)
    for name, idx in ac.placements(n).items():
        rows.append((name, ac.plant(base[0], idx, ac.OUTSIDE_DIV), base[1]))
        rows.append((name + " (denominator)", base[0], ac.plant(base[1], idx, ac.OUTSIDE_DIV)))
    with modes(gpu, jit=gpu.JIT_SYNC, fusion=True):
        before = gpu.engine_stats()["specialised_launches"]
        for label, ra, rb in rows:
            r = dv(gpu, ra).v1s1("MULT_S", 2.0).v2s0("DIV", dv(gpu, rb)).v1s0("ABS").v1s0("SQRT").v1s1("VID_S", 3.0)
            got = r.to_float32()
            w = ac.ref_div(np.full_like(ra, 3.0), ac.ref_sqrt(np.abs(ac.ref_div(ac._mul(ra, 2.0), rb))))
            check(ac.first_difference_by_class(got, w, names, "fused chain") if label == "classes" else ac.first_difference(got, w, f"fused chain, {label}"))
        assert gpu.engine_stats()["specialised_launches"] - before >= len(rows)


# ------------------------------------------------------------------------------------------------ 4. rolled and peeled loop kernels
def test_rolled_loop_that_divides_and_takes_a_root(gpu):
    """tests/test_gpu_rolled.py's running-sum loop with a square root in its body; out-of-range elements enter in the first iterations
    (in front of the loop), in the middle of it and in the last ones, through the numerator and through the shared rate."""
    n, iterations = 30011, 70
    rng = np.random.default_rng(11)
    xs = [ac.f32(rng.uniform(0.5, 1.5, n)) for _ in range(iterations)]
    shared = ac.f32(rng.uniform(0.0, 1.0, n))
    where = ac.placements(n)
    for j, name in ((0, "every_slot"), (1, "last_element"), (iterations // 2, "one_per_wave"), (iterations - 2, "first_and_last_lane"), (iterations - 1, "exactly_one")):
        xs[j] = ac.plant(xs[j], shifted(where[name], j, n) if name != "last_element" else where[name], ac.f32([2.0 ** 50, 1e-30, 0.0, 2.0 ** -49, 3e38]))
    shared = ac.plant(shared, where["middle_wave"], ac.f32([-2.0]))               # 1 + shared/2 = 0
    shared = ac.plant(shared, shifted(where["first_and_last_lane"], 8, n), ac.f32([2.0 ** 50]))     # denominator 2^49
    a = [0.3 + 0.01 * j for j in range(iterations)]
    b = [1.0 - 0.005 * j for j in range(iterations)]
    run, want = None, []
    for j, x in enumerate(xs):
        t = ac.ref_sqrt(np.abs(ac.ref_discount(ac._mul(x, a[j]), shared, 0.5)))
        run = t if run is None else ac._add(run, t)
        want.append(ac._add(x, ac._mul(run, b[j])))

    def chain(dev, dshared):
        run, ys = None, []
        for j, x in enumerate(dev):
            t = x.v1s1("MULT_S", a[j]).v2s1("DISCOUNT", dshared, 0.5).v1s0("ABS").v1s0("SQRT")
            run = t if run is None else run.v2s0("ADD", t)
            ys.append(x.v2s1("ADDPRODUCT_VS", run, b[j]))
        return ys
    launches = {}
    with modes(gpu, fusion=True):
        dshared = dv(gpu, shared)
        dev = [dv(gpu, x) for x in xs]
        for jit, name in ((gpu.JIT_OFF, "segments"), (gpu.JIT_SYNC, "discovery"), (gpu.JIT_SYNC, "rolled")):
            with modes(gpu, jit=jit):
                if name == "segments":
                    gpu.purge()
                with gpu.holding():
                    ys = chain(dev, dshared)
                before = gpu.pool_stats().n_kernel_launches
                gpu.flush()
                launches[name] = gpu.pool_stats().n_kernel_launches - before
                for j, y in enumerate(ys):
                    check(ac.first_difference(y.to_float32(), want[j], f"{name}: iteration {j}"))
                del ys
    assert launches["rolled"] < launches["segments"] and launches["rolled"] <= 6, launches


def test_peeled_loop_with_planted_elements(gpu):
    """tests/test_gpu_rolled.py's head-loop-tail chain (swaption backward induction: a DISCOUNT per period, a division by the numeraire
    in the tail) as ONE kernel; zero / huge denominators and out-of-range numerators enter in the head, inside the loop and in the tail."""
    n, periods = 50_021, 40
    rng = np.random.default_rng(77)
    libors = [ac.f32(rng.uniform(0.005, 0.04, n)) for _ in range(periods)]
    num = ac.f32(rng.uniform(1.0, 1.3, n))
    strike, delta = 0.02, 0.5
    where = ac.placements(n)
    libors[periods - 1] = ac.plant(libors[periods - 1], where["every_slot"], ac.f32([-2.0, 2.0 ** 50, np.float32(strike)]))      # head: den 0 / 2^49, numerator 0
    libors[periods // 2] = ac.plant(libors[periods // 2], shifted(where["one_per_wave"], 1, n), ac.f32([-2.0, 2.0 ** 50, -2.0 ** 60]))
    libors[0] = ac.plant(libors[0], where["last_element"], ac.f32([-2.0]))
    num = ac.plant(num, where["first_and_last_lane"], ac.f32([0.0, 2.0 ** 48, 1e-40, np.inf]))                                   # tail
    value = None
    for p in range(periods - 1, -1, -1):
        payoff = ac._mul(ac._add(libors[p], np.full(n, -np.float32(strike), dtype=np.float32)), delta)
        value = ac.ref_discount(payoff if value is None else ac._add(value, payoff), libors[p], delta)
    with np.errstate(all="ignore"):
        floored = np.where(np.isnan(value), value, np.maximum(value, np.float32(0.0)))
        floored = np.where(floored == 0, np.float32(0.0), floored)                   # Math.max(-0.0f, 0.0f) = +0.0f
    want = ac.ref_div(floored, num)

    def chain(dev, dnum):
        value = None
        for p in range(periods - 1, -1, -1):
            payoff = dev[p].v1s1("SUB_S", strike).v1s1("MULT_S", delta)
            value = (payoff if value is None else value.v2s0("ADD", payoff)).v2s1("DISCOUNT", dev[p], delta)
        return value.v1s1("FLOOR_S", 0.0).v2s0("DIV", dnum)
    launches = {}
    with modes(gpu, fusion=True):
        dev = [dv(gpu, x) for x in libors]
        dnum = dv(gpu, num)
        for jit, name in ((gpu.JIT_OFF, "segments"), (gpu.JIT_SYNC, "discovery"), (gpu.JIT_SYNC, "peeled")):
            with modes(gpu, jit=jit):
                if name == "segments":
                    gpu.purge()
                with gpu.holding():
                    got = chain(dev, dnum)
                before = gpu.pool_stats().n_kernel_launches
                gpu.flush()
                launches[name] = gpu.pool_stats().n_kernel_launches - before
                check(ac.first_difference(got.to_float32(), want, name))
    assert launches["segments"] >= 4 and launches["peeled"] == 1, launches


# ------------------------------------------------------------------------------------------------ 5. merged chains, shared denominator
def test_merged_chains_with_a_shared_denominator(gpu, oracle):
    """tests/test_gpu_merged_chains.py's swaptions of one exercise date: the chains of a merged launch discount by the same rate, so the
    denominator is prepared once (div_prepare_discount / ueval_div_prepared: every merged launch is generated with the shared denominator,
    merged_chains_engine.hpp: merge_families, and tests/test_jit_source_cpu.py pins that such a source divides through ueval_div_prepared).  A numerator that leaves the range in ONE chain only (its
    first payoff is zero), denominators that leave it for all chains (zero, 2^49)."""
    n, dates, tenors = 8197, (60, 60), (60, 40, 30, 20, 14, 12)
    prods = [(d, periods, 0.01 + 0.002 * k + 0.0005 * d) for d in range(len(dates)) for k, periods in enumerate(tenors)]
    rng = np.random.default_rng(3)
    L_h = [[ac.f32(rng.uniform(-0.01, 0.05, n)) for _ in range(n_vec)] for n_vec in dates]
    num_h = [ac.f32(rng.uniform(0.9, 1.4, n)) for _ in dates]
    where = ac.placements(n)
    for i, (d, periods, rate) in enumerate(prods):        # a chain starts at vector periods-1 with the payoff (L - rate)/2: zero where L == rate
        L_h[d][periods - 1] = ac.plant(L_h[d][periods - 1], shifted(where["one_per_wave"], 3 * i, n), ac.f32([rate]))
    for d in range(len(dates)):
        L_h[d][5] = ac.plant(L_h[d][5], where["every_slot"], ac.f32([-2.0, 2.0 ** 50]))
        L_h[d][17] = ac.plant(L_h[d][17], np.concatenate([where["last_element"], where["exactly_one"]]), ac.f32([-2.0]))

    def swaption(L, numeraire, periods, rate):
        value = None
        for p in range(periods - 1, -1, -1):
            payoff = L[p].v1s1("SUB_S", rate).v1s1("MULT_S", 0.5)
            value = (payoff if value is None else value.v2s0("ADD", payoff)).v2s1("DISCOUNT", L[p], 0.5)
        return value.v1s1("FLOOR_S", 0.0).v2s0("DIV", numeraire)

    def swaption_oracle(d, periods, rate):
        o, value = oracle, None
        for p in range(periods - 1, -1, -1):
            payoff = o.f_v1s1("MULT_S", o.f_v1s1("SUB_S", L_h[d][p], rate), 0.5)
            value = o.f_v2s1("DISCOUNT", payoff if value is None else o.f_v2s0("ADD", value, payoff), L_h[d][p], 0.5)
        return o.f_v2s0("DIV", o.f_v1s1("FLOOR_S", value, 0.0), num_h[d])
    with np.errstate(all="ignore"):
        want = [swaption_oracle(*q) for q in prods]
    # the planted numerators are zero in their own chain only
    first = [ac._mul(ac._add(L_h[d][periods - 1], np.full(n, -np.float32(rate), dtype=np.float32)), 0.5) for d, periods, rate in prods]
    assert all((f == 0).sum() >= n // 256 - 1 for f in first)
    with modes(gpu, fusion=False):
        L = [[dv(gpu, x) for x in row] for row in L_h]
        num = [dv(gpu, x) for x in num_h]
        eager = [swaption(L[d], num[d], periods, rate).to_float32() for d, periods, rate in prods]
        for k in range(len(prods)):
            check(ac.first_difference(eager[k], want[k], f"eager, chain {k}"))
        with modes(gpu, fusion=True, jit=gpu.JIT_SYNC):
            prev_hold = gpu.fusion_hold(2)
            try:
                gpu.purge()
                for round_ in range(3):
                    values = [swaption(L[d], num[d], periods, rate) for d, periods, rate in prods]
                    before = gpu.engine_stats()
                    for v in values:
                        v.moments()                        # the first call runs everything pending; from the second round on as merged launches
                    after = gpu.engine_stats()
                    for k, (d, periods, rate) in enumerate(prods):
                        check(ac.first_difference(values[k].to_float32(), want[k], f"round {round_}, chain {k} (date {d}, {periods} periods)"))
                    if round_ >= 1:
                        assert after["merged_launches"] > before["merged_launches"], "no merged launch"
                        assert after["merged_chains"] - before["merged_chains"] == len(prods)
                    del values
            finally:
                gpu.fusion_hold(prev_hold)


# ------------------------------------------------------------------------------------------------ 6. scalars on the specialised tier
@pytest.mark.parametrize("form", ["DIV_S", "VID_S"])
def test_scalars_at_the_gates_on_both_tiers(gpu, form):
    """The wave-uniform operand is range-tested on the scalar unit (div_range_key): an out-of-range scalar over in-range vectors must
    send every wave to the full expansion — and an in-range one must not hide an out-of-range element."""
    x, _, names = class_rows("unary")
    inside = ac.in_range_vector(100_003, 9)
    wa, wb = ac.from_bits([ac.WITNESS[0]])[0], ac.from_bits([ac.WITNESS[1]])[0]
    for s in ac.SCALARS + [float(wb if form == "DIV_S" else wa), 2.0 ** 47, -(2.0 ** -48)]:
        rows = [("classes", x, x, x), ("in-range vector", inside, inside, inside)]
        res = run_both_tiers(gpu, form, s, rows)
        for jit, out in res.items():
            check(ac.first_difference_by_class(out[0][0], reference(form, s, x, x, x), names, f"{form} {s!r}, jit mode {jit}"))
            check(ac.first_difference(out[1][0], reference(form, s, inside, inside, inside), f"{form} {s!r}, jit mode {jit}, in-range vector"))


# ------------------------------------------------------------------------------------------------ 7. pow
def pow_program(gpu, s):
    p = gpu.Program(1)
    w = p.op("POW_S", p.op("MULT_S", 0, s=1.0), s=s)
    p.output(w)
    return p.compile()


def run_pow(gpu, s, vectors):
    res = {}
    for jit, tier in ((gpu.JIT_OFF, 0), (gpu.JIT_SYNC, 1)):
        with modes(gpu, jit=jit):
            p = pow_program(gpu, s)
            assert p.tier()[0] == tier
            res[jit] = [p.run([[dv(gpu, v)]])[0][0][0].to_float32() for v in vectors]
    return res


@functools.lru_cache(maxsize=None)
def pow_reference(s):
    (x,), names = ac.concatenated(ac.pow_bases())
    return x, names, ac.allowed_pow(x, s)


@pytest.mark.parametrize("s", list(ac.POW_SPECIAL) + ac.pow_exponent_neighbours() + [0.0, 1.0, 1.0 / 3.0, 7.0, -3.0, np.inf, np.nan])
def test_pow_special_exponents_and_their_neighbours(gpu, s):
    x, names, (A, B) = pow_reference(s)
    big, _, bnames = class_rows("unary")
    res = run_pow(gpu, s, [x, big])
    for jit, (got, got_big) in res.items():
        check(ac.first_not_allowed(got, x, A, B, f"POW_S {s!r}, jit mode {jit}"))
        if s in ac.POW_EXACT:                  # correctly rounded forms: bit equality on every class
            with np.errstate(all="ignore"):
                want = {2.0: ac._mul(big, big), -1.0: ac.ref_div(np.ones_like(big), big),
                        0.5: np.where(np.isneginf(big), np.float32(np.inf), np.abs(ac.ref_sqrt(big)))}[s]
            check(ac.first_difference_by_class(got_big, want, bnames, f"POW_S {s!r}, jit mode {jit}"))
    check(ac.first_difference(res[gpu.JIT_OFF][1], res[gpu.JIT_SYNC][1], f"POW_S {s!r}: the two tiers"))


@pytest.mark.parametrize("s", [1.5, 2.5])
def test_pow_half_integer_exponents_in_mixed_waves(gpu, s):
    """Waves of positive bases with a single base that is not positive (-inf, -0, negative, zero, NaN): the library path for that lane."""
    n = 8197
    base = np.abs(ac.in_range_vector(n, 12, 1e-3, 1e3))
    not_positive = ac.f32([-np.inf, -0.0, -1.0, 0.0, np.nan, -1e-45, -2.25])
    vectors = [ac.plant(base, idx + shift, np.roll(not_positive, -shift)) for shift in (0, 1) for idx in
               (v[v + 1 < n] for v in ac.placements(n).values())]
    assert len(vectors) == 12
    res = run_pow(gpu, s, vectors)
    A0, B0 = ac.allowed_pow(base, s)
    for k, v in enumerate(vectors):
        changed = np.flatnonzero(ac.bits(v) != ac.bits(base))
        A, B = A0.copy(), B0.copy()
        A[changed], B[changed] = ac.allowed_pow(v[changed], s)
        for jit, out in res.items():
            check(ac.first_not_allowed(out[k], v, A, B, f"POW_S {s}, jit mode {jit}, vector {k}"))


# ------------------------------------------------------------------------------------------------ 8. FAST math mode
def ulps_between(a, b):
    ia, ib = ac.f32(a).view(np.int32).astype(np.int64), ac.f32(b).view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("op", ["EXP", "LOG"])
def test_fast_math_mode(gpu, op):
    classes = ac.exp_arguments() if op == "EXP" else ac.log_arguments()
    wide = classes["ordinary"] if op == "EXP" else np.concatenate([classes["all_exponents"], classes["denormals"]])
    special = classes["specials"]
    A, B = (ac.allowed_exp if op == "EXP" else ac.allowed_log)(wide)
    SA, _ = (ac.allowed_exp if op == "EXP" else ac.allowed_log)(special)
    a, b, names = class_rows("binary")
    with modes(gpu, math=gpu.MATH_FAST):
        for jit, tier in ((gpu.JIT_OFF, 0), (gpu.JIT_SYNC, 1)):
            with modes(gpu, jit=jit):
                p = gpu.Program(2)
                p.output(p.op(op, 0))
                p.output(p.op("SQRT", p.op("ABS", p.op("DIV", p.op("MULT_S", 0, s=1.0), 1))))
                p.compile()
                assert p.tier()[0] == tier
                got = p.run([[dv(gpu, wide), dv(gpu, wide)]])[0][0][0].to_float32()
                normal = np.isfinite(A) & (np.abs(A) >= 2.0 ** -126)
                worst = ulps_between(got[normal], A[normal]).max()
                assert worst <= 2, f"{op} fast, jit mode {jit}: {worst} ulp"
                got = p.run([[dv(gpu, special), dv(gpu, special)]])[0][0][0].to_float32()
                plain = np.isfinite(SA) & (SA != 0) & (np.abs(SA) >= 2.0 ** -126)
                assert (ulps_between(got[plain], SA[plain]) <= 2).all()
                check(ac.first_difference(got[~plain], SA[~plain], f"{op} fast, jit mode {jit}: special values"))
                # division and square root are exact in this mode too
                got = p.run([[dv(gpu, a), dv(gpu, b)]])[0][0][1].to_float32()
                check(ac.first_difference_by_class(got, ac.ref_sqrt(np.abs(ac.ref_div(a, b))), names, f"fast mode, jit mode {jit}: sqrt(|a / b|)"))


# ------------------------------------------------------------------------------------------------ 9. strided sweep over all bit patterns
SWEEP_STRIDE = 257
SWEEP = [("SQRT", None), ("INVERT", None), ("DIV_S", 3.0), ("VID_S", 3.0), ("POW_S", 0.5), ("POW_S", -1.0), ("POW_S", 1.5), ("POW_S", 2.5),
         ("POW_S", -2.0), ("POW_S", 4.0), ("EXP", None)]
EXACT_IN_SWEEP = {("SQRT", None), ("INVERT", None), ("DIV_S", 3.0), ("VID_S", 3.0), ("POW_S", 0.5), ("POW_S", -1.0)}


@pytest.mark.parametrize("op,s", SWEEP)
def test_strided_sweep_over_all_bit_patterns(gpu, oracle, op, s):
    """Every 257th fp32 bit pattern from a seeded offset (1.67e7 arguments) on the specialised tier against the oracle: bit for bit for
    the correctly rounded operations, within the tolerance of tests/test_gpu_parity_ops.py (1 ulp on at most 1e-5 of the elements, two
    fp64 libraries may differ in their last bit) for exp and the fp64 forms of pow."""
    offset = int(np.random.default_rng(SWEEP.index((op, s))).integers(0, SWEEP_STRIDE))
    x = np.arange(offset, 1 << 32, SWEEP_STRIDE, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        want = oracle.f_v1s0(op, x) if s is None else oracle.f_v1s1(op, x, s)
    with modes(gpu, jit=gpu.JIT_SYNC):
        p = gpu.Program(1)
        p.output(p.op(op, 0) if s is None else p.op(op, 0, s=s))
        p.compile()
        assert p.tier()[0] == 1
        got = p.run([[dv(gpu, x)]])[0][0][0].to_float32()
    if (op, s) in EXACT_IN_SWEEP:
        check(ac.first_difference(got, want, f"{op} {s}"))
    else:
        assert (np.isnan(got) == np.isnan(want)).all()
        d = ulps_between(got, want)
        d[np.isnan(want)] = 0
        assert d.max() <= 1 and (d > 0).mean() <= 1e-5, f"{op} {s}: max {d.max()} ulp, {(d > 0).sum()} of {d.size} differ"
