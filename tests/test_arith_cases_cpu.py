"""tests/arith_cases.py itself (every generator really produces its class — an edit cannot hollow one out unnoticed) and the oracle
on those classes: division, square root and the composite dividing operations bit for bit against numpy fp64 narrowed once (a
flush-to-zero or fused-multiply-add build of the oracle would show here), pow / exp / log within the stated contract against mpmath."""
import numpy as np
import pytest

import arith_cases as ac


def test_ragged_sizes_are_those_of_the_parity_test():
    import test_gpu_parity_ops
    assert ac.RAGGED_SIZES == test_gpu_parity_ops.RAGGED_SIZES


def test_gate_straddlers_sit_on_both_sides_of_every_gate():
    for gates in (ac.DIV_GATES, ac.SQRT_GATES):
        g = ac.gate_values(gates)
        assert g.size == 20 and np.unique(ac.bits(g)).size == 20
        for gate in gates:
            for sign in (1.0, -1.0):
                side = g[np.sign(g) == sign]
                assert (np.abs(side) == gate).sum() == 1
                below, above = np.abs(side) < gate, np.abs(side) > gate
                near = (np.abs(side) > gate / 1.001) & (np.abs(side) < gate * 1.001)
                assert (below & near).sum() == 2 and (above & near).sum() == 2
    classes = ac.gate_straddlers()
    assert set(classes) == {"gate_numerator", "gate_denominator", "gate_both"}
    lo, hi = ac.DIV_GATES
    inside = lambda v: (np.abs(v) >= lo) & (np.abs(v) < hi)
    a, b = classes["gate_numerator"]
    assert inside(b).all() and (~inside(a)).sum() >= 40 and inside(a).sum() >= 40
    a, b = classes["gate_denominator"]
    assert inside(a).all() and (~inside(b)).sum() >= 40 and inside(b).sum() >= 40
    a, b = classes["gate_both"]
    assert a.size == 400 and (~inside(a) & ~inside(b)).sum() >= 60 and (inside(a) & inside(b)).sum() >= 60


def test_exponent_grid_holds_every_pair_of_exponents_and_every_kind_of_number():
    a, b = ac.exponent_grid()["exponent_grid"]
    assert a.size == 256 * 256 * 16
    ea, eb = (ac.bits(a) >> 23) & 0xff, (ac.bits(b) >> 23) & 0xff
    assert np.unique(ea.astype(np.int64) * 256 + eb).size == 65536
    for v in (a, b):
        assert (v == 0).sum() > 100 and np.isinf(v).sum() > 100 and np.isnan(v).sum() > 100
        assert ((v != 0) & (np.abs(v) < 2.0 ** -126)).sum() > 1000                  # denormals
        assert np.signbit(v).sum() > v.size // 3 and (~np.signbit(v)).sum() > v.size // 3
        m = ac.bits(v) & 0x7fffff
        for fixed in (0, 1, 0x400000, 0x7fffff):
            assert (m == fixed).sum() > v.size // 10
        assert np.unique(m).size > 100000                                           # the random ones
    # a second call gives the same operands
    a2, b2 = ac.exponent_grid()["exponent_grid"]
    assert (ac.bits(a) == ac.bits(a2)).all() and (ac.bits(b) == ac.bits(b2)).all()


def test_every_case_of_div_scale_has_its_members():
    cases = ac.div_scale_cases()
    assert set(cases) == set(ac.div_scale_case_of(np.ones(1), np.ones(1)))
    for name, (a, b) in cases.items():
        member = ac.div_scale_case_of(a, b)[name]
        assert member.sum() >= 256, f"{name}: {member.sum()} of {a.size} operand pairs are in the case"
        assert np.signbit(a).any() and (~np.signbit(a)).any(), name
    a, b = cases["quotient_ties_between_denormals"]
    q = ac.ref_div(a, b)
    assert (np.abs(q) < 2.0 ** -126).all() and ((ac.bits(q) & 1) == 0).all()             # ties go to the even neighbour
    a, b = cases["quotient_rounds_up_to_smallest_normal"]
    assert (np.abs(ac.ref_div(a, b)) == np.float32(2.0 ** -126)).all()


def test_hard_quotients_are_in_the_range_they_name():
    lo, hi = ac.DIV_GATES
    classes = ac.hard_quotients()
    assert len(classes) == 4 * len(ac.RESCALINGS)
    for name, (a, b) in classes.items():
        inside = (np.abs(a) >= lo) & (np.abs(a) < hi) & (np.abs(b) >= lo) & (np.abs(b) < hi)
        if "just_outside" in name:
            assert (~inside).all(), name
        else:
            assert inside.all(), name
        if "low_edge" in name:
            assert (np.abs(a) < lo * 8).all() or (np.abs(b) < lo * 8).all(), name
        if "high_edge" in name:
            assert (np.abs(a) >= hi / 8).all() or (np.abs(b) >= hi / 8).all(), name
    a, b = classes["hardest_midpoint_middle"]
    q = np.abs(a.astype(np.float64)) / b.astype(np.float64) * 2.0 ** 24              # the fp64 quotient: an odd integer but for 2^-24 relative
    assert a.size > 5000 and (np.round(q) % 2 == 1).all() and (np.abs(q - np.round(q)) * b * 2.0 ** 23 <= 3.5).all() and (q != np.round(q)).any()
    a, b = classes["witness_middle"]
    assert set(ac.bits(np.abs(a))) == {ac.WITNESS[0]} and set(ac.bits(b)) == {ac.WITNESS[1]}
    # next to a representable quotient / next to a midpoint: the fp64 quotient is within 2^-22 relative of the 24- or 25-bit number
    for name, step in (("near_representable_middle", 2.0 ** -23), ("near_midpoint_middle", 2.0 ** -24)):
        a, b = classes[name]
        q = a.astype(np.float64) / b.astype(np.float64)
        off = np.abs(q / step - np.round(q / step)) * step / q
        assert (off < 2.0 ** -22).all() and a.size == 20000
        assert (off < 2.0 ** -28).sum() > 5000                   # the k = 0 third: within a few hundredths of an ulp
        if "midpoint" in name:
            assert (np.round(q / step)[off < 2.0 ** -28] % 2 == 1).mean() > 0.8


def test_hard_square_roots():
    classes = ac.hard_square_roots()
    lo, hi = ac.SQRT_GATES
    fast = lambda v: (v >= lo) & (v < hi)
    for kind in ("square", "midpoint_square"):
        assert fast(classes[f"{kind}_middle"]).all() and fast(classes[f"{kind}_low_gate"]).all() and fast(classes[f"{kind}_high_gate"]).all()
        below, above = classes[f"{kind}_below_low_gate"], classes[f"{kind}_above_high_gate"]
        assert (~fast(below)).sum() > 1000 and fast(below).sum() > 1000
        assert (~fast(above)).all() and (~fast(classes[f"{kind}_tiny"])).all() and (~fast(classes[f"{kind}_huge"])).all()
        e = (ac.bits(classes[f"{kind}_middle"]) >> 23) & 1
        assert (e == 0).sum() > 1000 and (e == 1).sum() > 1000                       # even and odd exponents
    r = ac.ref_sqrt(classes["exact_squares"]).astype(np.float64)
    assert (r * r == classes["exact_squares"]).all() and (~fast(classes["exact_squares"])).sum() > 1000
    d = classes["denormals"]
    assert d.size > 30000 and (d > 0).all() and (d < 2.0 ** -126).all() and ac.bits(d).max() > 0x7ff000
    assert classes["gates"].size == 20


def test_discount_denominators_leave_the_range_while_the_rate_stays_inside():
    lo, hi = ac.DIV_GATES
    seen = set()
    for name, r, s in ac.discount_denominators():
        assert ((np.abs(r) >= lo) & (np.abs(r) < hi) | (r == 0)).all(), name
        with np.errstate(all="ignore"):
            den = ac.narrow(1.0 + ac.narrow(r.astype(np.float64) * np.float64(np.float32(s))).astype(np.float64))
        outside = ~((np.abs(den) >= lo) & (np.abs(den) < hi))
        if name == "denominator_tiny_product":
            assert (den == 1.0).all()
        else:
            assert outside.any(), name
        seen |= {"zero"} if (den == 0).any() else set()
        seen |= {"inf"} if np.isinf(den).any() else set()
        seen |= {"nan"} if np.isnan(den).any() else set()
        seen |= {"cancel"} if (np.abs(den) == np.float32(2.0 ** -24)).any() else set()
        seen |= {"at_gate"} if (np.abs(den) == np.float32(2.0 ** 48)).any() and (np.abs(den) == ac.neighbours(2.0 ** 48, 1)[0]).any() else set()
    assert seen == {"zero", "inf", "nan", "cancel", "at_gate"}


def test_pow_exp_classes():
    bases = ac.pow_bases()
    e = (ac.bits(bases["positive_normals"]) >> 23) & 0xff
    assert set(e) == set(range(1, 255)) and (bases["positive_normals"] > 0).all()
    assert (bases["denormals"] < 2.0 ** -126).all() and (bases["denormals"] > 0).all() and (bases["negatives"] < 0).all()
    assert len(ac.pow_exponent_neighbours()) == 16 and not set(ac.pow_exponent_neighbours()) & set(ac.POW_SPECIAL)
    x = ac.exp_arguments()
    t = x["overflow_threshold"].astype(np.float64)
    assert (np.exp(t) < 2.0 ** 128).sum() > 100 and (np.exp(t) >= 2.0 ** 128).sum() > 100
    d = np.exp(x["denormal_results"].astype(np.float64))
    assert ((d < 2.0 ** -126) & (d > 2.0 ** -150)).sum() > 10000 and (d >= 2.0 ** -126).any() and (d < 2.0 ** -150).any()
    assert (np.abs(x["tiny_arguments"]) < 2.0 ** -23).all() and (np.abs(x["tiny_arguments"]) < 2.0 ** -25).sum() > 150


def test_placements_cover_every_slot_and_the_ragged_end():
    n = 100000
    p = ac.placements(n)
    slots = set()
    for i in p["every_slot"]:
        quad, comp = divmod(int(i), 4)
        part = (quad // ac.FM_BLOCK) % 2
        slots.add(part * 4 + comp)
    assert slots == set(range(8))
    assert np.unique(p["every_slot"] // 4 % ac.FM_BLOCK // ac.WAVE + p["every_slot"] // 2048 * 4).size == p["every_slot"].size      # one plant per wave
    lanes = p["first_and_last_lane"] // 4 % ac.WAVE
    assert set(lanes) == {0, ac.WAVE - 1}
    assert p["last_element"].tolist() == [n - 1] and p["exactly_one"].size == 1 and p["middle_wave"].size == 1
    assert p["one_per_wave"].size == -(-n // ac.FM_BLOCK)
    for size in ac.RAGGED_SIZES + ac.LARGE_SIZES:
        for name, idx in ac.placements(size).items():
            assert ((idx >= 0) & (idx < size)).all(), (size, name)
    base = ac.in_range_vector(n, 1)
    planted = ac.plant(base, p["one_per_wave"], ac.OUTSIDE_DIV)
    changed = np.flatnonzero(ac.bits(planted) != ac.bits(base))
    assert (changed == p["one_per_wave"]).all()
    lo, hi = ac.DIV_GATES
    assert ((np.abs(base) >= lo) & (np.abs(base) < hi)).all()
    assert not ((np.abs(ac.OUTSIDE_DIV) >= lo) & (np.abs(ac.OUTSIDE_DIV) < hi)).any()
    assert not ((ac.OUTSIDE_SQRT >= ac.SQRT_GATES[0]) & (ac.OUTSIDE_SQRT < ac.SQRT_GATES[1])).any()


# ---------------------------------------------------------------------------------------- the oracle on these classes
def test_oracle_division_is_the_correctly_rounded_quotient(oracle):
    (a, b), names = ac.concatenated(ac.binary_classes())
    assert a.size > 1_300_000
    with np.errstate(all="ignore"):
        assert ac.first_difference_by_class(oracle.f_v2s0("DIV", a, b), ac.ref_div(a, b), names, "DIV") is None
        c = np.roll(a, 12345)
        assert ac.first_difference_by_class(oracle.f_v3s0("ADDRATIO", c, a, b), ac.ref_addratio(c, a, b), names, "ADDRATIO") is None
        assert ac.first_difference_by_class(oracle.f_v3s0("SUBRATIO", c, a, b), ac.ref_subratio(c, a, b), names, "SUBRATIO") is None


def test_oracle_unary_and_scalar_division(oracle):
    (x,), names = ac.concatenated(ac.unary_classes())
    with np.errstate(all="ignore"):
        assert ac.first_difference_by_class(oracle.f_v1s0("SQRT", x), ac.ref_sqrt(x), names, "SQRT") is None
        assert ac.first_difference_by_class(oracle.f_v1s0("INVERT", x), ac.ref_div(np.ones_like(x), x), names, "INVERT") is None
        for s in ac.SCALARS:
            sv = np.full_like(x, np.float32(s))
            assert ac.first_difference_by_class(oracle.f_v1s1("DIV_S", x, s), ac.ref_div(x, sv), names, f"DIV_S {s!r}") is None
            assert ac.first_difference_by_class(oracle.f_v1s1("VID_S", x, s), ac.ref_div(sv, x), names, f"VID_S {s!r}") is None


def test_oracle_discount(oracle):
    (x,), names = ac.concatenated(ac.unary_classes())
    a = np.roll(x, 999)
    with np.errstate(all="ignore"):
        for s in (0.5, -1.0, 1.0 / 3.0, 2.0 ** 24, 2.0 ** 90, np.inf):
            assert ac.first_difference_by_class(oracle.f_v2s1("DISCOUNT", a, x, s), ac.ref_discount(a, x, s), names, f"DISCOUNT {s!r}") is None
        for name, r, s in ac.discount_denominators():
            num = np.resize(ac.HARMLESS, r.size)
            assert ac.first_difference(oracle.f_v2s1("DISCOUNT", num, r, s), ac.ref_discount(num, r, s), name) is None


@pytest.mark.parametrize("s", list(ac.POW_SPECIAL) + ac.pow_exponent_neighbours() + [0.0, 1.0, 1.0 / 3.0, -0.5, 7.0, -3.0, np.inf, -np.inf, np.nan])
def test_oracle_pow_meets_its_contract(oracle, s):
    (x,), names = ac.concatenated(ac.pow_bases())
    A, B = ac.allowed_pow(x, s)
    with np.errstate(all="ignore"):
        got = oracle.f_v1s1("POW_S", x, s)
    assert ac.first_not_allowed(got, x, A, B, f"POW_S {s!r}") is None
    if s in ac.POW_EXACT:                       # exactly rounded forms: the answer is unique
        assert (ac.bits(A) == ac.bits(B)).all()
    assert (ac.bits(A) != ac.bits(B)).mean() < 1e-2


def test_oracle_exp_and_log_meet_their_contract(oracle):
    (x,), _ = ac.concatenated(ac.exp_arguments())
    with np.errstate(all="ignore"):
        assert ac.first_not_allowed(oracle.f_v1s0("EXP", x), x, *ac.allowed_exp(x), "EXP") is None
    (x,), _ = ac.concatenated(ac.log_arguments())
    with np.errstate(all="ignore"):
        assert ac.first_not_allowed(oracle.f_v1s0("LOG", x), x, *ac.allowed_log(x), "LOG") is None
