"""Shared between tests/test_arith_cases_cpu.py and tests/test_gpu_arith_gates.py: fp32 operands that sit where the hand-written
arithmetic of csrc/fm_device_math.hpp decides something (the range gates of the short division chain and of the fast square root,
the cases of v_div_scale_f32 / v_div_fixup_f32, the special exponents of pow_all, the thresholds of exp), and references that do
not go through oracle/: numpy fp64 narrowed once for division and square root (53 >= 2·24 + 2: that IS the correctly rounded fp32
result, denormals included), mpmath for pow / exp / log.  Every generator is seeded and returns NAMED arrays, so that a failure
says which class broke."""
import functools

import numpy as np

DIV_GATES = (2.0 ** -48, 2.0 ** 48)            # div_pair_in_range is used while every operand lies in [2^-48, 2^48)
SQRT_GATES = (2.0 ** -63, 2.0 ** 63)           # sqrt_fast_path while 2^-63 <= a < 2^63
POW_SPECIAL = (2.0, 0.5, -1.0, 3.0, 4.0, -2.0, 1.5, 2.5)      # exponents with code of their own in pow_all
POW_EXACT = (2.0, 0.5, -1.0)                   # … whose forms are correctly rounded: bit equality on every base
RAGGED_SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 100000]   # test_gpu_parity_ops.py
LARGE_SIZES = [262_144 + 3, 1_000_003]         # several workgroups; full passes and a ragged tail
WITNESS = (0x3f80d000, 0x3fe45d41)             # first mantissa pair the chain gets wrong without its Newton step (fm_device_math.hpp)


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.int64) & 0xffffffff, dtype=np.int64).astype(np.uint32).view(np.float32)


def bits(x):
    return f32(x).view(np.uint32)


def neighbours(x, k=2):
    """x and its k neighbours on each side (by magnitude), positive x: 2k+1 values in ascending order."""
    b = int(bits([x])[0])
    return from_bits(b + np.arange(-k, k + 1))


def scale2(x, e):
    """x·2^e, exact while the result stays a normal number."""
    return np.ldexp(f32(x), np.asarray(e, dtype=np.int32)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ references
def narrow(x64):
    with np.errstate(all="ignore"):
        return np.asarray(x64, dtype=np.float64).astype(np.float32)


def ref_div(a, b):
    with np.errstate(all="ignore"):
        return narrow(f32(a).astype(np.float64) / f32(b).astype(np.float64))


def ref_sqrt(a):
    with np.errstate(all="ignore"):
        return narrow(np.sqrt(f32(a).astype(np.float64)))


def _mul(a, b):          # fp32 product, rounded once (the fp64 product of two fp32 numbers is exact)
    with np.errstate(all="ignore"):
        return narrow(f32(a).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64))


def _add(a, b):          # fp32 sum, rounded once (double rounding is innocuous for a sum as well)
    with np.errstate(all="ignore"):
        return narrow(f32(a).astype(np.float64) + f32(b).astype(np.float64))


def ref_discount(a, r, s):
    """fl(a / fl(1 + fl(r·s))), s narrowed to fp32 first — every step rounds once, no fused multiply-add."""
    den = _add(np.ones_like(f32(r)), _mul(r, float(s)))
    return ref_div(a, den)


def ref_addratio(acc, x, y):
    return _add(acc, ref_div(x, y))


def ref_subratio(acc, x, y):
    return _add(acc, -ref_div(x, y))


def same_bits(got, want):
    """Element-wise: same fp32 bit pattern, or both NaN (payload ignored)."""
    got, want = f32(got), f32(want)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


def first_difference(got, want, what):
    """None, or a message naming the first element of `got` that is not `want` (bits)."""
    ok = same_bits(got, want)
    if ok.all():
        return None
    i = int(np.flatnonzero(~ok)[0])
    return (f"{what}: {int((~ok).sum())} of {ok.size} differ; first at {i}: got 0x{int(bits(got)[i]):08x} ({f32(got)[i]!r}), "
            f"want 0x{int(bits(want)[i]):08x} ({f32(want)[i]!r})")


# ---- pow / exp / log against mpmath -----------------------------------------------------------------------------
_F32_MAX = float(np.finfo(np.float32).max)


def _allowed_pair(t, mp):
    """For a finite, non-zero true value t (mpf): the fp32 values a result may take — the correctly rounded one, or either neighbour
    when t lies within 2 fp64 ulps of the midpoint between them.  Returned as two floats (equal when the answer is unique)."""
    sign = -1.0 if t < 0 else 1.0
    m = abs(t)
    if m >= mp.mpf(2) ** 128:
        return sign * np.inf, sign * np.inf
    d = float(m)                                            # nearest double
    f = np.float32(min(d, _F32_MAX))
    lo = f if mp.mpf(float(f)) <= m else np.nextafter(f, np.float32(0))
    with np.errstate(over="ignore"):
        hi = np.nextafter(lo, np.float32(np.inf))           # inf above the largest float
    hi_value = mp.mpf(2) ** 128 if np.isinf(hi) else mp.mpf(float(hi))
    lo_value = mp.mpf(float(lo))
    if lo_value == m:
        return sign * float(lo), sign * float(lo)
    mid = (lo_value + hi_value) / 2
    if m == mid:                                            # an exact tie (a short power): representable in fp64, narrowed to even
        r = float(lo) if (int(bits([lo])[0]) & 1) == 0 else float(hi)
        return sign * r, sign * r
    ulp64 = mp.mpf(2) ** (max(int(mp.floor(mp.log(m, 2))), -1022) - 52)
    if abs(m - mid) <= 2 * ulp64:
        return sign * float(lo), sign * float(hi)
    r = float(lo) if m < mid else float(hi)
    return sign * r, sign * r


def _java_pow_special(x, y):
    """Math.pow where no real power exists or the value is 0 / inf / NaN / exactly 1; None: take the real power."""
    if y == 0.0:
        return 1.0
    if np.isnan(x) or np.isnan(y):
        return np.nan
    if np.isinf(y):
        if abs(x) == 1.0:
            return np.nan
        return np.inf if (abs(x) > 1.0) == (y > 0) else 0.0
    y_int = float(y).is_integer()
    y_odd = y_int and abs(y) < 2.0 ** 53 and int(y) % 2 == 1
    if x == 0.0 or np.isinf(x):
        big = np.isinf(x) == (y > 0)                        # |result| infinite
        sign = -1.0 if (np.signbit(x) and y_odd) else 1.0
        return sign * (np.inf if big else 0.0)
    if x < 0 and not y_int:
        return np.nan
    return None


@functools.lru_cache(maxsize=None)
def _mp():
    import mpmath
    mpmath.mp.prec = 240
    return mpmath.mp


def allowed_pow(x, s):
    """(A, B): fp32 arrays; `(float)Math.pow((double)x, (double)(float)s)` must be A or B (or NaN where both are NaN)."""
    mp = _mp()
    x = f32(x)
    y = float(np.float32(s))
    A, B = np.empty_like(x), np.empty_like(x)
    for i, xv in enumerate(x.astype(np.float64)):
        r = _java_pow_special(xv, y)
        if r is None:
            t = mp.power(mp.mpf(abs(xv)), mp.mpf(y))
            if xv < 0 and int(y) % 2 != 0:
                t = -t
            a, b = _allowed_pair(t, mp)
        else:
            a = b = r
        A[i], B[i] = a, b
    return A, B


def allowed_exp(x):
    mp = _mp()
    x = f32(x)
    A, B = np.empty_like(x), np.empty_like(x)
    for i, xv in enumerate(x.astype(np.float64)):
        if np.isnan(xv):
            a = b = np.nan
        elif np.isinf(xv):
            a = b = np.inf if xv > 0 else 0.0
        elif xv == 0.0:
            a = b = 1.0
        elif xv < -110.0:
            a = b = 0.0
        else:
            a, b = _allowed_pair(mp.exp(mp.mpf(xv)), mp)
        A[i], B[i] = a, b
    return A, B


def allowed_log(x):
    mp = _mp()
    x = f32(x)
    A, B = np.empty_like(x), np.empty_like(x)
    for i, xv in enumerate(x.astype(np.float64)):
        if np.isnan(xv) or xv < 0:
            a = b = np.nan
        elif xv == 0.0:
            a = b = -np.inf
        elif np.isinf(xv):
            a = b = np.inf
        elif xv == 1.0:
            a = b = 0.0
        else:
            a, b = _allowed_pair(mp.log(mp.mpf(xv)), mp)
        A[i], B[i] = a, b
    return A, B


def within_allowed(got, A, B):
    return same_bits(got, A) | same_bits(got, B)


def first_not_allowed(got, x, A, B, what):
    ok = within_allowed(got, A, B)
    if ok.all():
        return None
    i = int(np.flatnonzero(~ok)[0])
    return (f"{what}: {int((~ok).sum())} of {ok.size} outside the contract; first at {i}: argument 0x{int(bits(x)[i]):08x} ({f32(x)[i]!r}) "
            f"got 0x{int(bits(got)[i]):08x} ({f32(got)[i]!r}), allowed {A[i]!r} / {B[i]!r}")


# ------------------------------------------------------------------------------------------------ operand classes
HARMLESS = f32([1.0, -3.0, 0.7, -1.5e10, 2.5e-9, 1.0000001, -0.99999994, 12345.678])       # inside every gate


def gate_values(gates):
    """Every gate, its two neighbours on each side, both signs."""
    v = np.concatenate([neighbours(g, 2) for g in gates])
    return np.concatenate([v, -v])


def gate_straddlers(gates=DIV_GATES):
    """name -> (a, b): the gate values as numerator (over harmless denominators), as denominator, and as both."""
    g = gate_values(gates)
    gg, hh = np.meshgrid(g, HARMLESS, indexing="ij")
    ga, gb = np.meshgrid(g, g, indexing="ij")
    return {"gate_numerator": (gg.ravel().copy(), hh.ravel().copy()),
            "gate_denominator": (hh.ravel().copy(), gg.ravel().copy()),
            "gate_both": (ga.ravel().copy(), gb.ravel().copy())}


MANTISSAS = (0, 1, 0x400000, 0x7fffff, None)        # None: random


def exponent_grid(seed=1, per_pair=16):
    """All 256 x 256 pairs of biased exponents, `per_pair` mantissa pairs each out of {0, 1, 0x400000, 0x7fffff, random}², signs
    mixed: zeros, denormals, normals, infinities and NaNs all fall out of the grid.  256·256·16 = 1 048 576 quotients."""
    rng = np.random.default_rng(seed)
    ea, eb, k = np.meshgrid(np.arange(256), np.arange(256), np.arange(per_pair), indexing="ij")
    ea, eb, k = ea.ravel(), eb.ravel(), k.ravel()
    combo = (k + 7 * ea + 3 * eb) % 25

    def mant(which):
        table = np.array([0, 1, 0x400000, 0x7fffff, 0], dtype=np.int64)
        m = table[which]
        rnd = rng.integers(0, 1 << 23, which.size)
        return np.where(which == 4, rnd, m)
    ma, mb = mant(combo % 5), mant(combo // 5)
    sa, sb = rng.integers(0, 2, ea.size), rng.integers(0, 2, ea.size)
    a = from_bits((sa << 31) | (ea << 23) | ma)
    b = from_bits((sb << 31) | (eb << 23) | mb)
    return {"exponent_grid": (a, b)}


def exponent_of(x):
    """Unbiased exponent of a normal number (biased - 127); denormals and zero: -127, infinities and NaN: 128."""
    return ((bits(x) >> 23) & 0xff).astype(np.int64) - 127


def div_scale_case_of(a, b):
    """The cases of v_div_scale_f32 / v_div_fixup_f32 that the comment above div_pair_in_range lists, as boolean masks."""
    a, b = f32(a), f32(b)
    ea, eb = exponent_of(a), exponent_of(b)
    fin_a, fin_b = np.isfinite(a), np.isfinite(b)
    normal_a = fin_a & (np.abs(a) >= 2.0 ** -126)
    normal_b = fin_b & (np.abs(b) >= 2.0 ** -126)
    with np.errstate(all="ignore"):
        q = np.abs(a.astype(np.float64) / b.astype(np.float64))
        r = narrow(q)
        tie = q * 2.0 ** 150 % 2 == 1
    proper = normal_a & fin_b & (b != 0) & (a != 0)
    return {
        "exponent_difference_ge_96": normal_a & normal_b & (ea - eb >= 96),
        "exponent_difference_le_m96": normal_a & normal_b & (ea - eb <= -96),
        "denominator_denormal": fin_b & (b != 0) & ~normal_b & fin_a & (a != 0),
        "denominator_above_2p126": fin_b & (np.abs(b) > 2.0 ** 126) & fin_a & (a != 0),
        "quotient_denormal": proper & (q < 2.0 ** -126) & (r != 0) & (r < 2.0 ** -126),
        "quotient_ties_between_denormals": proper & (q < 2.0 ** -126) & tie,
        "quotient_rounds_up_to_smallest_normal": proper & (q < 2.0 ** -126) & (r == np.float32(2.0 ** -126)),
        "quotient_underflows_to_zero": proper & (q != 0) & (r == 0),
        "numerator_below_2m103": fin_a & (a != 0) & (np.abs(a) < 2.0 ** -103) & normal_b,
        "quotient_overflows": fin_a & fin_b & (b != 0) & np.isinf(r),
        "zero_over_zero": (a == 0) & (b == 0),
        "inf_over_inf": np.isinf(a) & np.isinf(b),
        "x_over_zero": fin_a & (a != 0) & (b == 0),
        "nan_anywhere": np.isnan(a) | np.isnan(b),
    }


def div_scale_cases(seed=2, per_case=512):
    """name -> (a, b): one vector per case of div_scale_case_of, built for that case (random members, both signs)."""
    rng = np.random.default_rng(seed)
    n = per_case

    def normal(e_lo, e_hi):           # random normal numbers with unbiased exponent in [e_lo, e_hi]
        e = rng.integers(e_lo + 127, e_hi + 128, n)
        return from_bits((rng.integers(0, 2, n) << 31) | (e << 23) | rng.integers(0, 1 << 23, n))

    def denormal():
        return from_bits((rng.integers(0, 2, n) << 31) | rng.integers(1, 1 << 23, n))
    out = {}
    b = normal(-126, 30)
    out["exponent_difference_ge_96"] = (scale2(np.abs(b), rng.integers(96, 98, n)) * np.where(rng.integers(0, 2, n) == 1, -1, 1).astype(np.float32), b)
    a = normal(-126, 30)
    out["exponent_difference_le_m96"] = (a, scale2(np.abs(a), rng.integers(96, 98, n)))
    out["denominator_denormal"] = (normal(-126, 0), denormal())
    out["denominator_above_2p126"] = (normal(-20, 127), normal(126, 127))
    out["quotient_denormal"] = (normal(-100, -96), normal(32, 45))
    # quotient exactly half-way between two denormals: (2j+1)·2^-150 = (2j+1)·2^-90 / 2^60, also with a common factor 3
    j = rng.integers(0, 1 << 21, n)
    odd = (2 * j + 1).astype(np.float64)
    three = np.where(np.arange(n) % 2 == 0, 1.0, 3.0)
    sign = np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0)
    out["quotient_ties_between_denormals"] = (f32(sign * odd * three * 2.0 ** -90), f32(three * 2.0 ** 60))
    # quotients in [2^-126 - 2^-150, 2^-126): they round UP to the smallest normal number
    top = from_bits(np.full(n, 0x3fffffff))                                              # 2 - 2^-23
    e = rng.integers(-60, 0, n)
    a_up = scale2(top, e)
    b_up = scale2(np.ones(n, dtype=np.float32), e + 127)
    b_up[1::2] = from_bits(bits(b_up[1::2]).astype(np.int64) - 1)                       # a denominator one ulp smaller: just above the tie
    out["quotient_rounds_up_to_smallest_normal"] = (a_up, b_up)
    out["quotient_underflows_to_zero"] = (normal(-126, -100), normal(60, 127))
    out["numerator_below_2m103"] = (np.concatenate([normal(-126, -104)[: n // 2], denormal()[: n - n // 2]]), normal(-126, -80))
    out["quotient_overflows"] = (normal(40, 127), normal(-126, -90))
    z = np.where(rng.integers(0, 2, n) == 1, -0.0, 0.0).astype(np.float32)
    out["zero_over_zero"] = (z, z[::-1].copy())
    i = np.where(rng.integers(0, 2, n) == 1, -np.inf, np.inf).astype(np.float32)
    out["inf_over_inf"] = (i, i[::-1].copy())
    out["x_over_zero"] = (np.concatenate([normal(-126, 127)[: n // 2], denormal()[: n - n // 2]]), z)
    nan = np.full(n, np.nan, dtype=np.float32)
    other = np.concatenate([normal(-126, 127)[: n - 8], f32([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45, 3e38])])
    out["nan_anywhere"] = (np.concatenate([nan, other, nan]), np.concatenate([other, nan, nan]))
    for name, (a, b) in out.items():            # no case depends on a sign: flip every third numerator and every fifth denominator
        a, b = a.copy(), b.copy()
        a[2::3], b[4::5] = -a[2::3], -b[4::5]
        out[name] = (a, b)
    return out


RESCALINGS = {"middle": (0, 0), "numerator_low_edge": (-48, 46), "numerator_high_edge": (46, -48), "both_low_edge": (-48, -48),
              "both_high_edge": (46, 46), "just_outside_low": (-50, 0), "just_outside_high": (0, 48)}


def hardest_midpoints(rng, n):
    """(a, b) with a / b = Q/2^25 + r/(2^25·b), Q odd with 25 bits and r in {±1, ±3}: the quotients closest to the midpoint of two
    fp32 numbers that exist (relative distance ≈ 2^-49) — a chain whose error before the last rounding exceeds that gets them wrong.
    For an odd 24-bit b, Q = -r·b^-1 mod 2^25 makes b·Q + r divisible by 2^25; a = (b·Q + r)/2^25 is an integer below 2^24."""
    a, b = [], []
    for B in (rng.integers(1 << 22, 1 << 23, n) * 2 + 1).tolist():
        for r in (1, -1, 3, -3):
            Q = (-r * pow(B, -1, 1 << 25)) % (1 << 25)
            A = (B * Q + r) >> 25
            if Q >= 1 << 24:                                 # then 2^22 <= A < 2^24
                a.append(A); b.append(B)
    sign = np.where(rng.integers(0, 2, len(a)) == 1, -1.0, 1.0)
    return f32(np.array(a, dtype=np.float64) * sign * 2.0 ** -22), f32(np.array(b, dtype=np.float64) * 2.0 ** -23)       # a in [1, 4), b in [1, 2)


def hard_quotients(seed=3, n=20000):
    """name -> (a, b): a = nextafter^k(fl(q·b)), k in {-1, 0, 1}, for random b in [1, 2) and q in [1, 2) with 24 significant bits
    (a / b lands next to a representable number) or 25 (next to the midpoint of two; for k = 0 within a hundredth of an ulp), the hardest midpoint quotients there are (hardest_midpoints) and the documented witness pair of the short
    chain — each rescaled by powers of two to the middle of the range [2^-48, 2^48) and to its inner edges (a in [1, 4), b in [1, 2))."""
    rng = np.random.default_rng(seed)
    over = 64                                       # of 64·n random pairs keep the n whose product q·b is closest to an fp32 number
    b_all = from_bits(0x3f800000 | rng.integers(0, 1 << 23, over * n))
    q24_all = from_bits(0x3f800000 | rng.integers(0, 1 << 23, over * n)).astype(np.float64)
    k = rng.integers(-1, 2, n)
    base = {}
    for name, q_all in (("near_representable", q24_all), ("near_midpoint", q24_all + 2.0 ** -24)):
        product = q_all * b_all.astype(np.float64)                                       # exact: 25 + 24 bits
        keep = np.argsort(np.abs(product - narrow(product).astype(np.float64)) / product)[:n]
        keep = keep[rng.permutation(n)]
        a = narrow(product[keep])
        base[name] = (from_bits(bits(a).astype(np.int64) + k), b_all[keep])
    base["hardest_midpoint"] = hardest_midpoints(rng, n // 4)
    wa, wb = from_bits([WITNESS[0]]), from_bits([WITNESS[1]])
    base["witness"] = (np.repeat(np.concatenate([wa, -wa]), 64), np.repeat(np.concatenate([wb, wb]), 64))
    out = {}
    for name, (a, b_) in base.items():
        for rname, (sa, sb) in RESCALINGS.items():
            out[f"{name}_{rname}"] = (scale2(a, sa), scale2(b_, sb))
    return out


def hard_square_roots(seed=4, n=20000):
    """name -> a: k² and (k + 1/2)² rounded to fp32 and their two neighbours for random 24-bit k (roots next to a representable number /
    next to a midpoint; k² in [2^46, 2^48) covers both exponent parities), moved over the range and to both gates of the fast path;
    the denormal range by stride; the gate values themselves."""
    rng = np.random.default_rng(seed)
    k = rng.integers(1 << 23, 1 << 24, n).astype(np.float64)
    d = rng.integers(-1, 2, n)
    out = {}
    for name, sq in (("square", k * k), ("midpoint_square", k * k + k)):
        a = from_bits(bits(narrow(sq)).astype(np.int64) + d)                              # in [2^46, 2^48]
        for rname, e in (("middle", -46), ("low_gate", -46 - 63), ("below_low_gate", -46 - 64), ("high_gate", 15), ("above_high_gate", 17),
                         ("odd_shift", -47), ("tiny", -46 - 100), ("huge", 78)):
            out[f"{name}_{rname}"] = scale2(a, e)
    out["exact_squares"] = np.concatenate([f32(np.arange(1, 4096, dtype=np.float64) ** 2) * np.float32(4.0 ** e) for e in (-40, -31, 0, 20, 31)])
    out["denormals"] = from_bits(np.arange(1, 1 << 23, 257))
    out["gates"] = gate_values(SQRT_GATES)
    out["specials"] = f32([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -1e-45, 1e-45, 3.4028235e38, 1.1754944e-38, 1.0, 4.0, 2.0])
    return out


def discount_denominators():
    """List of (name, r, s): 1 + r·s is zero, tiny by cancellation, at / next to 2^48, infinite or NaN, while r itself lies inside the
    division's range (or is zero) — the gate has to look at the denominator, not at r.  s is the scalar of the launch."""
    one_minus = from_bits([0x3f7fffff])[0]           # 1 - 2^-24
    one_plus = from_bits([0x3f800001])[0]            # 1 + 2^-23
    # (a non-zero 1 + r·s is a multiple of 2^-24: it cannot fall below the lower gate, only cancel to zero)
    cases = [
        ("denominator_zero", f32([-0.5, -0.25, -0.5, -0.125]), 2.0),                       # only -0.5·2 = -1; the others are in range
        ("denominator_cancels", f32([-one_minus, -one_plus, -1.0, 0.5]), 1.0),            # 2^-24, -2^-23, 0, 1.5
        ("denominator_at_2p48", np.concatenate([neighbours(2.0 ** 24, 2), -neighbours(2.0 ** 24, 2)]), 2.0 ** 24),
        ("denominator_infinite", f32([2.0 ** 47, -2.0 ** 47, 1.0, 2.0 ** -40]), 2.0 ** 90),
        ("denominator_nan_zero_times_inf", f32([0.0, -0.0, 1.0, -1.0]), np.inf),
        ("denominator_nan_scalar", f32([1.0, 2.0, 3.0, 4.0]), np.nan),
        ("denominator_tiny_product", f32([2.0 ** -47, -2.0 ** -47, 2.0 ** -30, 1.0]), 2.0 ** -90),   # 1 + r·s = 1: IN range, though r·s is not
    ]
    return cases


def pow_bases(seed=5, per_exponent=6):
    """name -> x: positive normal numbers over all exponents, denormals, negatives (integers and fractions), and the special values."""
    rng = np.random.default_rng(seed)
    e = np.repeat(np.arange(1, 255), per_exponent)
    table = np.array([0, 1, 0x400000, 0x7fffff], dtype=np.int64)
    m = np.where(np.arange(e.size) % per_exponent < 4, table[np.arange(e.size) % 4], rng.integers(0, 1 << 23, e.size))
    pos = from_bits((e << 23) | m)
    return {"positive_normals": pos,
            "denormals": from_bits(np.concatenate([np.arange(1, 40), rng.integers(1, 1 << 23, 400), [0x7fffff, 0x400000]])),
            "negatives": np.concatenate([-pos[::7], f32([-1.0, -2.0, -3.0, -0.5, -1.5, -1e-45, -3.4028235e38, -16777216.0, -16777215.0])]),
            "near_one": from_bits(0x3f800000 + np.arange(-300, 301)),
            "specials": f32([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])}


def pow_exponent_neighbours():
    """The fp32 neighbours of every special exponent of pow_all: they must take the library path."""
    out = []
    for s in POW_SPECIAL:
        b = int(bits([s])[0])
        out += [float(from_bits([b - 1])[0]), float(from_bits([b + 1])[0])]
    return out


EXP_OVERFLOW = 88.72284          # exp(x) overflows fp32 above this


def exp_arguments(seed=6):
    rng = np.random.default_rng(seed)
    return {"overflow_threshold": from_bits(int(bits([EXP_OVERFLOW])[0]) + np.arange(-400, 401)),
            "denormal_results": np.concatenate([f32(np.linspace(-103.99, -87.33, 12000)), -neighbours(87.33655, 40), -neighbours(103.97208, 40), -neighbours(103.27893, 40)]),
            "tiny_arguments": np.concatenate([scale2(np.ones(100, dtype=np.float32), -np.arange(24, 124)), -scale2(np.ones(100, dtype=np.float32), -np.arange(24, 124)),
                                              from_bits(rng.integers(1, 1 << 23, 100))]),
            "ordinary": f32(rng.uniform(-87.0, 88.0, 4000)),
            "specials": f32([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 89.0, -104.0, -110.0, -150.0, 3.4028235e38, -3.4028235e38])}


def log_arguments(seed=7):
    rng = np.random.default_rng(seed)
    return {"all_exponents": pow_bases(seed)["positive_normals"],
            "denormals": from_bits(np.concatenate([np.arange(1, 40), rng.integers(1, 1 << 23, 400)])),
            "near_one": from_bits(0x3f800000 + np.arange(-300, 301)),
            "specials": f32([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, -1e-45])}


SCALARS = [*(float(v) for v in gate_values(DIV_GATES)), 0.0, -0.0, 1e-45, -1e-40, np.inf, -np.inf, np.nan, 2.0 ** 60, 2.0 ** -60, -2.0 ** 60, 1.0 / 3.0, 3.0]


# ------------------------------------------------------------------------------------------------ placement
FM_BLOCK, WAVE = 256, 64         # threads per workgroup, lanes per wave; a lane holds 4 consecutive elements per tile part


def element_index(tile, part, wave, lane, component, parts=2):
    """Index of one element of a lane's E = 4·parts elements: part t of tile `tile` is a run of 1024 elements, 4 per thread."""
    return (((tile * parts + part) * FM_BLOCK) + wave * WAVE + lane) * 4 + component


def placements(n, seed=8):
    """name -> indices (< n, possibly empty) at which to plant out-of-range elements into an in-range vector of n elements."""
    rng = np.random.default_rng(seed + n)
    out = {}
    # every slot of a lane's 8 elements, each in a wave of its own (the fallback is wave-wide: a slot it forgets stays wrong)
    out["every_slot"] = np.array([element_index(w // 4, (w % 8) // 4, w % 4, (7 * w + 3) % WAVE, w % 4) for w in range(16)]
                                 + [element_index(4 + w // 4, ((w + 4) % 8) // 4, w % 4, (11 * w) % WAVE, (w + 1) % 4) for w in range(16)])
    out["first_and_last_lane"] = np.array([element_index(9, 0, 1, 0, 0), element_index(9, 1, 2, WAVE - 1, 3), element_index(10, 0, 0, 0, 2), element_index(10, 1, 3, WAVE - 1, 1)])
    out["middle_wave"] = np.array([(n // 2) | 1])
    out["last_element"] = np.array([n - 1])
    out["exactly_one"] = rng.integers(0, max(n, 1), 1)
    w = np.arange(0, max(n, 1), FM_BLOCK)
    out["one_per_wave"] = w + (37 * (w // FM_BLOCK)) % FM_BLOCK
    return {k: np.unique(v[(v >= 0) & (v < n)]).astype(np.int64) for k, v in out.items()}


def plant(base, positions, values):
    """Copy of `base` with `values` (cycled) written at `positions`."""
    out = f32(base).copy()
    if len(positions):
        out[positions] = np.resize(f32(values), len(positions))
    return out


def in_range_vector(n, seed, lo=0.25, hi=4.0):
    """n values with magnitude in [lo, hi), both signs: well inside every gate."""
    rng = np.random.default_rng(seed)
    return f32(rng.uniform(lo, hi, n) * np.where(rng.integers(0, 2, n) == 1, -1.0, 1.0))


OUTSIDE_DIV = f32([2.0 ** 48, -2.0 ** 60, 2.0 ** -49, -1e-30, 0.0, np.inf, np.nan, 1e-42, 3e38])       # outside [2^-48, 2^48)
OUTSIDE_SQRT = f32([2.0 ** 63, 2.0 ** -64, 1e-30, 3e38, 1e-42, 0.0, -1.0, np.inf, np.nan])             # outside [2^-63, 2^63)


def concatenated(classes):
    """dict name -> tuple of arrays  →  (tuple of concatenated arrays, [(name, start, stop)]): many classes through ONE launch."""
    names, cols, at = [], None, 0
    for name, arrays in classes.items():
        arrays = arrays if isinstance(arrays, tuple) else (arrays,)
        cols = [[] for _ in arrays] if cols is None else cols
        for c, a in zip(cols, arrays):
            c.append(f32(a))
        names.append((name, at, at + arrays[0].size))
        at += arrays[0].size
    return tuple(np.concatenate(c) for c in cols), names


def first_difference_by_class(got, want, names, what):
    for name, lo, hi in names:
        msg = first_difference(got[lo:hi], want[lo:hi], f"{what}, class {name}")
        if msg:
            return msg
    return None


def binary_classes():
    """Every (a, b) class of the division, under one naming."""
    out = {}
    out.update(gate_straddlers(DIV_GATES))
    out.update({f"scale_{k}": v for k, v in div_scale_cases().items()})
    out.update({f"hard_{k}": v for k, v in hard_quotients().items()})
    out.update(exponent_grid())
    return out


def unary_classes():
    """Every single-vector class: arguments of SQRT / INVERT / DIV_S / VID_S / POW_S."""
    out = {f"sqrt_{k}": v for k, v in hard_square_roots().items()}
    out["gates_div"] = gate_values(DIV_GATES)
    out.update({f"pow_{k}": v for k, v in pow_bases().items()})
    a, b = exponent_grid(per_pair=1)["exponent_grid"]
    out["all_exponents_mixed"] = np.concatenate([a, b])
    wa, wb = hard_quotients(n=2000)["witness_middle"]
    out["witness_numerator"], out["witness_denominator"] = wa, wb
    return out
