"""Catalogue of loop shapes, shared by tests/test_gpu_loop_shapes.py: recurrences whose pending graph is periodic, each chosen to
drive one path of the loop-kernel generator (csrc/jit.cpp: jit_generate_rolled_source, jit_generate_merged_source) or one condition of
the detector (csrc/loop_engine.hpp: Engine::detect_loop, plan_peel; csrc/merged_chains_engine.hpp: merge_families).

A shape is a PAIR of functions over the same data — `device(d)` records the recurrence on DeviceVectors with v1s0 … v3s0, `oracle(o, d)`
restates it with oracle.f_v* — and, next to them, the description the engine is meant to make of it (`expect`): what one line of
FMHIP_JIT_RECORD says (jit.cpp: jit_describe).  Both functions return {name: vector} of everything that keeps a handle; whatever else
they compute is dropped, as a caller drops its temporaries — which values keep a handle decides what a loop stores.

What the detector does with handles (loop_engine.hpp, detect_loop: out_needed / final_needed), since the shapes are built around it:
  * a value with a handle, or read later than the next iteration, is an OUTPUT of its position: stored in every iteration;
  * a FINAL value is one of the last iteration that only the operations BEHIND the loop read; with a handle of its own it would be an
    output — so the engine never asks a peeled kernel to store a final value (Peel::final_store is 0 in every description it makes);
  * a value without a handle that nobody reads does not exist: the last iteration of a shape is as long as its live values;
  * the loop starts where the detector's periodic stretch starts (behind the last operation of the first iteration that reads a leaf
    where the later ones read a carried value) and at the rotation with the fewest values crossing: its "iteration" is often a rotation
    of the recurrence's, and the rest of the last one runs behind the loop, reading one value of it — the `final=1` of most shapes below.
"""
import numpy as np

ITERATIONS = 24


def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


class Shape:
    """name, data(rng, n) -> dict, device(d) -> {name: DeviceVector}, oracle(o, d) -> {name: array}, expect: the recorded description
    (None: whether and how it rolls is the engine's business), exact: every operation correctly rounded (the oracle's bits)."""

    def __init__(self, name, data, device, oracle, expect, exact=True, plantable=()):
        self.name, self.data, self.device, self.oracle, self.expect, self.exact, self.plantable = name, data, device, oracle, expect, exact, plantable

    def __repr__(self):
        return self.name


def expect(period, globals=0, inputs=1, carried=1, final=0, out=0, elems=8, peel=True):
    return dict(period=period, globals=globals, inputs=inputs, carried=carried, final=final, out=out, elems=elems, peel=peel)


def uniform(rng, n, lo, hi, count=None):
    if count is None:
        return f32(rng.uniform(lo, hi, n))
    return [f32(rng.uniform(lo, hi, n)) for _ in range(count)]


def to_device(gpu, d):
    """The data of a shape with every array uploaded ONCE: an array that sits in two places is the same vector in both."""
    memo = {}

    def conv(x):
        if isinstance(x, np.ndarray):
            if id(x) not in memo:
                memo[id(x)] = gpu.DeviceVector.from_host(x)
            return memo[id(x)]
        if isinstance(x, list):
            return [conv(y) for y in x]
        return x
    return {k: conv(v) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ two_carried
def two_carried_data(rng, n, iterations=ITERATIONS):
    return {"s0": uniform(rng, n, 0.5, 1.5), "v0": uniform(rng, n, 0.5, 1.5), "x": uniform(rng, n, -0.5, 0.5, iterations),
            "y": uniform(rng, n, 0.0, 1.0, iterations), "b": [0.1 + 0.02 * j for j in range(iterations)], "scale": 2.0}


def two_carried_device(d):
    """s' = s.addProduct(x_j, v), v' = (v + b_j·(y_j − v)).floor(0): s keeps a handle in every iteration, v is read behind the loop only."""
    s, v, kept = d["s0"], d["v0"], {}
    for j, (x, y) in enumerate(zip(d["x"], d["y"])):
        s_next = s.v3s0("ADDPRODUCT", x, v)
        v = v.v2s1("ADDPRODUCT_VS", y.v2s0("SUB", v), d["b"][j]).v1s1("FLOOR_S", 0.0)
        s = s_next
        kept[f"s{j}"] = s
    kept["v_end"] = v.v1s1("MULT_S", d["scale"])
    return kept


def two_carried_oracle(o, d):
    s, v, kept = d["s0"], d["v0"], {}
    for j, (x, y) in enumerate(zip(d["x"], d["y"])):
        s_next = o.f_v3s0("ADDPRODUCT", s, x, v)
        v = o.f_v1s1("FLOOR_S", o.f_v2s1("ADDPRODUCT_VS", v, o.f_v2s0("SUB", y, v), d["b"][j]), 0.0)
        s = s_next
        kept[f"s{j}"] = s
    kept["v_end"] = o.f_v1s1("MULT_S", v, d["scale"])
    return kept


# ------------------------------------------------------------------------------------------------ final_not_carried
def final_not_carried_data(rng, n, iterations=ITERATIONS):
    return {"r0": uniform(rng, n, -0.5, 0.5), "x": uniform(rng, n, -0.5, 0.5, iterations), "a": [0.25 + 0.01 * j for j in range(iterations)]}


def final_not_carried_device(d):
    """run' = run + x_j (carried), w_j = run'·x_j, y_j = w_j + a_j (a handle each); z = (w_J − y_last) − y_5 with J the last iteration BUT ONE.
    The operations are scheduled consumers first (runtime.cpp: build_big), so z — which needs y_last — comes last; the detector's
    stretch starts at the second operation of the component and covers whole periods, so its loop ends one iteration before the
    component does: w_J is a value of the loop's last iteration that only an operation behind the loop reads — a final value that is not
    carried (register f0).  Because z also reads a value of an EARLIER iteration the component has no peeled form (plan_peel: make_op):
    the plain kernel stores f0 behind its loop and ordinary launches compute the rest.  (The issue's form — only the last w_j keeps a
    handle — makes no such value: the earlier w_j, read by nobody, do not exist, and a final value with a handle is an output.  This
    form leans on the scheduler's order and the detector's alignment; should either change, test_recorded_descriptions says so: it
    asks for a final position that is not a carried one, in a plain kernel.)"""
    run, kept, w = d["r0"], {}, []
    for j, x in enumerate(d["x"]):
        run = run.v2s0("ADD", x)
        w = (w + [run.v2s0("MULT", x)])[-2:]
        kept[f"y{j}"] = w[-1].v1s1("ADD_S", d["a"][j])
    kept["z"] = w[0].v2s0("SUB", kept[f"y{j}"]).v2s0("SUB", kept["y5"])
    return kept


def final_not_carried_oracle(o, d):
    run, kept, w = d["r0"], {}, []
    for j, x in enumerate(d["x"]):
        run = o.f_v2s0("ADD", run, x)
        w = (w + [o.f_v2s0("MULT", run, x)])[-2:]
        kept[f"y{j}"] = o.f_v1s1("ADD_S", w[-1], d["a"][j])
    kept["z"] = o.f_v2s0("SUB", o.f_v2s0("SUB", w[0], kept[f"y{j}"]), kept["y5"])
    return kept


# ------------------------------------------------------------------------------------------------ many_io
def many_io_data(rng, n, iterations=ITERATIONS):
    return {"c0": uniform(rng, n, 0.5, 1.5), "g0": uniform(rng, n, 0.0, 1.0), "g1": uniform(rng, n, 0.5, 1.5), "x": uniform(rng, n, 0.5, 1.5, iterations),
            "y": uniform(rng, n, -1.0, 1.0, iterations), "z": uniform(rng, n, -1.0, 1.0, iterations), "s": [0.5 - 0.01 * j for j in range(iterations)]}


def many_io_device(d):
    """Three inputs (x_j, y_j, z_j), three stored outputs, two loop-invariant vectors (six operations an iteration: their uses span
    more than the 128 nodes that make a vector a global, detect_loop: GLOBAL_SPAN)."""
    c, kept = d["c0"], {}
    for j, (x, y, z) in enumerate(zip(d["x"], d["y"], d["z"])):
        a = x.v2s1("DISCOUNT", d["g0"], 0.5)
        b = y.v2s0("MULT", d["g1"])
        c = c.v1s1("MULT_S", 0.5).v3s0("ADDPRODUCT", a, b)
        kept[f"p{j}"] = a.v2s0("ADD", z)
        kept[f"q{j}"] = b.v2s1("ADDPRODUCT_VS", z, d["s"][j])
        kept[f"c{j}"] = c
    return kept


def many_io_oracle(o, d):
    c, kept = d["c0"], {}
    for j, (x, y, z) in enumerate(zip(d["x"], d["y"], d["z"])):
        a = o.f_v2s1("DISCOUNT", x, d["g0"], 0.5)
        b = o.f_v2s0("MULT", y, d["g1"])
        c = o.f_v3s0("ADDPRODUCT", o.f_v1s1("MULT_S", c, 0.5), a, b)
        kept[f"p{j}"] = o.f_v2s0("ADD", a, z)
        kept[f"q{j}"] = o.f_v2s1("ADDPRODUCT_VS", b, z, d["s"][j])
        kept[f"c{j}"] = c
    return kept


# ------------------------------------------------------------------------------------------------ operand_slots
# Every line: (call shape, opcode, operands) with "c" = the carried value, "x" / "y" = the iteration's inputs, a float = the scalar.
# The carried value sits in each operand position in turn (runtime.cpp: variant_for's r1_pos / r2_pos → RolledBody::Op::x0 / x1 / x2).
SLOTS_3 = [(op, args) for op in ("ADDPRODUCT", "ADDRATIO", "SUBRATIO", "CHOOSE") for args in (("c", "x", "y"), ("x", "c", "y"), ("x", "y", "c"))]
SLOTS_2 = ([(op, args) for op in ("SUB", "DIV", "CAP", "FLOOR") for args in (("c", "x"), ("x", "c"))]
           + [(op, args) for op in ("ACCRUE", "DISCOUNT") for args in (("c", "y", 0.375), ("y", "c", 0.375))]
           + [("BUS_S", ("c", 1.75)), ("VID_S", ("c", 0.8125))])


def operand_slots_data(rng, n, iterations=ITERATIONS):
    # x, y and the carried value stay inside [0.5, 1.5]: no quotient is out of range unless something is planted
    return {"c0": uniform(rng, n, 0.5, 1.5), "x": uniform(rng, n, 0.5, 1.5, iterations), "y": uniform(rng, n, 0.5, 1.5, iterations)}


def _slots_device(table):
    def device(d):
        """Every operation of the table reads the carried value directly; the results are folded into the next carried value
        (Σ t_k / K kept inside [0.5, 1.25], plus c / 8), which keeps a handle in every iteration.  The LAST operation of an iteration
        reads the carried value too: the first iteration (which reads a leaf there) is aperiodic to its end, so the detector's loop
        starts where an iteration starts and the operations read c0 itself, not a copy of it made in front of them."""
        c, kept = d["c0"], {}
        for j, (x, y) in enumerate(zip(d["x"], d["y"])):
            acc = None
            for op, args in table:
                v = [{"c": c, "x": x, "y": y}[a] for a in args if isinstance(a, str)]
                s = [a for a in args if not isinstance(a, str)]
                if len(v) == 3: t = v[0].v3s0(op, v[1], v[2])
                elif len(v) == 2 and s: t = v[0].v2s1(op, v[1], s[0])
                elif len(v) == 2: t = v[0].v2s0(op, v[1])
                else: t = v[0].v1s1(op, s[0])
                acc = t if acc is None else acc.v2s0("ADD", t)
            c = acc.v1s1("MULT_S", 1.0 / len(table)).v1s1("FLOOR_S", 0.5).v1s1("CAP_S", 1.25).v2s1("ADDPRODUCT_VS", c, 0.125)
            kept[f"c{j}"] = c
        return kept
    return device


def _slots_oracle(table):
    def oracle(o, d):
        c, kept = d["c0"], {}
        for j, (x, y) in enumerate(zip(d["x"], d["y"])):
            acc = None
            for op, args in table:
                t = o.f_apply(op, *[{"c": c, "x": x, "y": y}[a] if isinstance(a, str) else a for a in args])
                acc = t if acc is None else o.f_v2s0("ADD", acc, t)
            c = o.f_v2s1("ADDPRODUCT_VS", o.f_v1s1("CAP_S", o.f_v1s1("FLOOR_S", o.f_v1s1("MULT_S", acc, 1.0 / len(table)), 0.5), 1.25), c, 0.125)
            kept[f"c{j}"] = c
        return kept
    return oracle


# ------------------------------------------------------------------------------------------------ library_math
def library_math_data(rng, n, iterations=ITERATIONS):
    return {"c0": uniform(rng, n, 0.5, 1.5), "x": uniform(rng, n, -0.5, 0.5, iterations)}


def library_math_device(d):
    """LOG, EXP, SQRT, POW_S(2.5), SIN, COS in one body: 4 elements per lane, the log table set up inside a loop kernel; the head (the
    first iteration) holds out-of-line library code, so there is no peeled form (plan_peel: make_op)."""
    c, kept = d["c0"], {}
    for j, x in enumerate(d["x"]):
        q = c.v1s0("LOG").v2s0("ADD", x).v1s0("EXP").v1s0("SQRT")
        p = q.v1s1("POW_S", 2.5)
        c = p.v1s0("SIN").v2s0("MULT", q.v1s0("COS")).v1s1("MULT_S", 0.5).v1s1("ADD_S", 1.0)
        kept[f"c{j}"] = c
    return kept


def library_math_oracle(o, d):
    c, kept = d["c0"], {}
    for j, x in enumerate(d["x"]):
        q = o.f_v1s0("SQRT", o.f_v1s0("EXP", o.f_v2s0("ADD", o.f_v1s0("LOG", c), x)))
        p = o.f_v1s1("POW_S", q, 2.5)
        c = o.f_v1s1("ADD_S", o.f_v1s1("MULT_S", o.f_v2s0("MULT", o.f_v1s0("SIN", p), o.f_v1s0("COS", q)), 0.5), 1.0)
        kept[f"c{j}"] = c
    return kept


# ------------------------------------------------------------------------------------------------ peeled_library_moments
def peeled_library_data(rng, n, iterations=ITERATIONS):
    return {"x": uniform(rng, n, 0.0, 1.0, iterations), "num": uniform(rng, n, 0.9, 1.4)}


def peeled_library_device(d):
    """value' = exp(0.3·(value + x_j)) behind a short head (the first iteration has no running value yet), floored and divided by a
    numeraire behind the loop: head, loop and tail in ONE launch at 4 elements per lane — a kernel that takes no moments itself."""
    value = None
    for x in d["x"]:
        value = (x if value is None else value.v2s0("ADD", x)).v1s1("MULT_S", 0.3).v1s0("EXP")
    return {"value": value.v1s1("FLOOR_S", 1.25).v2s0("DIV", d["num"])}


def peeled_library_oracle(o, d):
    value = None
    for x in d["x"]:
        value = o.f_v1s0("EXP", o.f_v1s1("MULT_S", x if value is None else o.f_v2s0("ADD", value, x), 0.3))
    return {"value": o.f_v2s0("DIV", o.f_v1s1("FLOOR_S", value, 1.25), d["num"])}


# ------------------------------------------------------------------------------------------------ long_head_reload
def long_head_data(rng, n, iterations=ITERATIONS):
    return {"a": uniform(rng, n, 0.5, 1.5), "b": uniform(rng, n, 0.5, 1.5), "x": uniform(rng, n, 0.005, 0.04, iterations), "num": uniform(rng, n, 1.0, 1.3)}


def long_head_device(d):
    """A head of nine operations (more than jit.cpp's HEAD_AHEAD = 6: the first iteration's loads are issued inside it); its value h
    keeps a handle AND is read behind the loop (stored by the head, read back by the tail behind a wait: pre_out, the reload); the tail's
    root and one value in its middle keep handles (post_out)."""
    a, b = d["a"], d["b"]
    h = a.v2s0("MULT", b).v1s1("ADD_S", 0.25).v2s0("DIV", b).v2s0("SUB", a).v1s1("MULT_S", 0.5).v2s0("ADD", b).v1s1("FLOOR_S", 0.75)
    value = h.v1s1("SUB_S", 0.5).v1s1("MULT_S", 0.125)
    for x in d["x"]:
        value = value.v2s0("ADD", x.v1s1("SUB_S", 0.02).v1s1("MULT_S", 0.5)).v2s1("DISCOUNT", x, 0.5)
    mid = value.v1s1("FLOOR_S", 0.0).v2s0("MULT", h)
    return {"h": h, "mid": mid, "root": mid.v2s0("DIV", d["num"])}


def long_head_oracle(o, d):
    a, b = d["a"], d["b"]
    h = o.f_v2s0("MULT", a, b)
    h = o.f_v2s0("DIV", o.f_v1s1("ADD_S", h, 0.25), b)
    h = o.f_v1s1("FLOOR_S", o.f_v2s0("ADD", o.f_v1s1("MULT_S", o.f_v2s0("SUB", h, a), 0.5), b), 0.75)
    value = o.f_v1s1("MULT_S", o.f_v1s1("SUB_S", h, 0.5), 0.125)
    for x in d["x"]:
        value = o.f_v2s1("DISCOUNT", o.f_v2s0("ADD", value, o.f_v1s1("MULT_S", o.f_v1s1("SUB_S", x, 0.02), 0.5)), x, 0.5)
    mid = o.f_v2s0("MULT", o.f_v1s1("FLOOR_S", value, 0.0), h)
    return {"h": h, "mid": mid, "root": o.f_v2s0("DIV", mid, d["num"])}


# ------------------------------------------------------------------------------------------------ scan chains and their variations
SCAN_ITERATIONS = 40       # 4 operations an iteration: the uses of `shared` must span 128 nodes for it to be a global (detect_loop: GLOBAL_SPAN)


def scan_data(rng, n, iterations=SCAN_ITERATIONS):
    return {"x": uniform(rng, n, 0.5, 1.5, iterations), "shared": uniform(rng, n, 0.0, 1.0), "a": [0.3 + 0.01 * j for j in range(iterations)],
            "b": [1.0 - 0.005 * j for j in range(iterations)]}


def _scan_device(keep):
    def device(d):
        """y_j = x_j + run_j·b_j with run_j = run_{j-1} + x_j·a_j / (1 + shared_j·0.5) (test_gpu_rolled.py: scan_chain); every y_j keeps a handle, and
        so does the term t_j of iteration `keep` (the detector then stores that position in EVERY iteration); shared_j is ONE loop-invariant vector unless the data gives a list."""
        run, kept = None, {}
        for j, x in enumerate(d["x"]):
            shared = d["shared"][j] if isinstance(d["shared"], list) else d["shared"]
            t = x.v1s1("MULT_S", d["a"][j])
            t = t.v2s1("DISCOUNT", shared, 0.5)
            run = t if run is None else run.v2s0("ADD", t)
            y = x.v2s1("ADDPRODUCT_VS", run, d["b"][j])
            kept[f"y{j}"] = y
            if keep == j: kept[f"t{j}"] = t
        return kept
    return device


def _scan_oracle(keep):
    def oracle(o, d):
        run, kept = None, {}
        for j, x in enumerate(d["x"]):
            shared = d["shared"][j] if isinstance(d["shared"], list) else d["shared"]
            t = o.f_v1s1("MULT_S", x, d["a"][j])
            t = o.f_v2s1("DISCOUNT", t, shared, 0.5)
            run = t if run is None else o.f_v2s0("ADD", run, t)
            y = o.f_v2s1("ADDPRODUCT_VS", x, run, d["b"][j])
            kept[f"y{j}"] = y
            if keep == j: kept[f"t{j}"] = t
        return kept
    return oracle


def aliased_a_data(rng, n, iterations=SCAN_ITERATIONS):
    d = scan_data(rng, n, iterations)
    d["x"][20] = d["x"][3]                       # the same vector is the input of iteration 3 and of iteration 20
    return d


def aliased_b_data(rng, n, iterations=SCAN_ITERATIONS):
    d = scan_data(rng, n, iterations)
    d["shared"] = uniform(rng, n, 0.0, 1.0, iterations)      # two inputs an iteration …
    d["shared"][7] = d["x"][7]                   # … and in iteration 7 the same vector sits in both slots
    return d


def aliased_c_data(rng, n, iterations=SCAN_ITERATIONS):
    d = scan_data(rng, n, iterations)
    d["x"][17] = d["shared"]                     # the loop-invariant vector is also iteration 17's own input
    return d


# ------------------------------------------------------------------------------------------------ limits of detect_loop
def _chain_data(n_carried, n_inputs, iterations):
    def data(rng, n):
        return {"c": uniform(rng, n, 0.5, 1.5, n_carried), "x": [uniform(rng, n, -0.5, 0.5, n_inputs) for _ in range(iterations)],
                "w": [[0.01 * (1 + (k + j) % 5) for k in range(max(n_carried, n_inputs))] for j in range(iterations)]}
    return data


def carried_device(d):
    """K carried values: c_k' = c'_{k-1} + c_k·w_k (c'_{-1} = x_j); the last one of every iteration keeps a handle."""
    c, kept = list(d["c"]), {}
    for j, xs in enumerate(d["x"]):
        prev = xs[0]
        for k in range(len(c)):
            c[k] = prev = prev.v2s1("ADDPRODUCT_VS", c[k], d["w"][j][k])
        kept[f"o{j}"] = prev
    return kept


def carried_oracle(o, d):
    c, kept = list(d["c"]), {}
    for j, xs in enumerate(d["x"]):
        prev = xs[0]
        for k in range(len(c)):
            c[k] = prev = o.f_v2s1("ADDPRODUCT_VS", prev, c[k], d["w"][j][k])
        kept[f"o{j}"] = prev
    return kept


def inputs_device(d):
    """M inputs an iteration: acc' = acc·0.5 + Σ_m x_{j,m}·w_m, one operation per input."""
    acc, kept = d["c"][0], {}
    for j, xs in enumerate(d["x"]):
        acc = acc.v1s1("MULT_S", 0.5)
        for m, x in enumerate(xs):
            acc = acc.v2s1("ADDPRODUCT_VS", x, d["w"][j][m])
        kept[f"o{j}"] = acc
    return kept


def inputs_oracle(o, d):
    acc, kept = d["c"][0], {}
    for j, xs in enumerate(d["x"]):
        acc = o.f_v1s1("MULT_S", acc, 0.5)
        for m, x in enumerate(xs):
            acc = o.f_v2s1("ADDPRODUCT_VS", acc, x, d["w"][j][m])
        kept[f"o{j}"] = acc
    return kept


UNARY_CYCLE = ("SQRT", "SQUARED", "INVERT", "INVERT", "ABS")


def _long_body(n_scalar, n_plain):
    """acc' = (acc + x_j) through n_scalar scalar operations and n_plain operations without one: period 1 + n_scalar + n_plain."""
    def ops(j):
        out = [("MULT_S", 1.0 - 0.001 * ((k + j) % 7)) if k % 2 == 0 else ("ADD_S", 0.001 * ((k + j) % 5)) for k in range(n_scalar)]
        return out + [(UNARY_CYCLE[k % len(UNARY_CYCLE)], None) for k in range(n_plain)]

    def device(d):
        acc, kept = d["c"][0], {}
        for j, xs in enumerate(d["x"]):
            acc = acc.v2s0("ADD", xs[0]).v1s1("FLOOR_S", 0.25)
            for op, s in ops(j):
                acc = acc.v1s0(op) if s is None else acc.v1s1(op, s)
            kept[f"o{j}"] = acc
        return kept

    def oracle(o, d):
        acc, kept = d["c"][0], {}
        for j, xs in enumerate(d["x"]):
            acc = o.f_v1s1("FLOOR_S", o.f_v2s0("ADD", acc, xs[0]), 0.25)
            for op, s in ops(j):
                acc = o.f_v1s0(op, acc) if s is None else o.f_v1s1(op, acc, s)
            kept[f"o{j}"] = acc
        return kept
    return device, oracle


def _limit(name, n_carried, n_inputs, iterations, device, oracle, exp):
    return Shape(name, _chain_data(n_carried, n_inputs, iterations), device, oracle, exp)


_scal48, _scal49 = _long_body(47, 0), _long_body(48, 0)          # (+ the FLOOR_S in front: 48 and 49 scalars an iteration)
_per128, _per129 = _long_body(40, 86), _long_body(40, 87)        # (+ ADD and FLOOR_S: periods 128 and 129)
_per12 = _long_body(5, 5)                                        # period 12

# loop_engine.hpp, detect_loop: `if (G > 8 || CI > 12 || CO > 12 || LI > 12 || LO > 12 || LO + CO == 0 || LS > 48) return false;`, MAX_PERIOD = 128,
# `if (n < 48) return false;`, MIN_ITERATIONS = 5 (`R < MIN_ITERATIONS - 1`: the loop itself starts at the SECOND periodic iteration).
# For the period-12 body none of these decides: with one stored value an iteration a component of up to 8 iterations (96 operations, 9 input
# and 8 output vectors) still fits ONE ordinary launch (fm_program.h: FM_MAX_OPS = 128, FM_MAX_OUT = 8) and is never handed to the detector;
# the ninth iteration's output makes it a large component, and its loop (7 iterations behind the head) is rolled.
PERIOD12_ROLLS, PERIOD12_TOO_SHORT = 9, 8
LIMITS_INSIDE = [
    _limit("carried_12", 12, 1, ITERATIONS, carried_device, carried_oracle, expect(12, carried=12, out=1)),
    _limit("inputs_12", 1, 12, ITERATIONS, inputs_device, inputs_oracle, expect(13, inputs=12, final=1, out=1, peel=False)),
    _limit("scalars_48", 1, 1, ITERATIONS, *_scal48, expect(49, final=1, out=1)),
    _limit("period_128", 1, 1, 8, *_per128, expect(128, final=1, out=1)),
    _limit("period12_shortest", 1, 1, PERIOD12_ROLLS, *_per12, expect(12, final=1, out=1)),
]
LIMITS_OUTSIDE = [
    _limit("carried_13", 13, 1, ITERATIONS, carried_device, carried_oracle, None),
    _limit("inputs_13", 1, 13, ITERATIONS, inputs_device, inputs_oracle, None),
    _limit("scalars_49", 1, 1, ITERATIONS, *_scal49, None),
    _limit("period_129", 1, 1, 8, *_per129, None),
    _limit("period12_one_fewer", 1, 1, PERIOD12_TOO_SHORT, *_per12, None),
]

# ------------------------------------------------------------------------------------------------ merged families
# (merged_chains_engine.hpp: merge_families) products of ONE exercise date: each reads a suffix of the date's vectors.  `kind`:
#   "swaption"     test_gpu_merged_chains.py: swaption / swaption_oracle, every DISCOUNT with that module's PERIOD;
#   "other_period" the same induction discounting with another period — its shared scalar differs from the family's: left out of it;
#   "no_discount"  value = (value + payoff)·L[p]: a shape without shared scalars.
OTHER_PERIOD = 0.25


def family_chain(kind, L, numeraire, periods, rate):
    from test_gpu_merged_chains import PERIOD, swaption
    if kind == "swaption":
        return swaption(L, numeraire, periods, rate)
    value = None
    for p in range(periods - 1, -1, -1):
        payoff = L[p].v1s1("SUB_S", rate).v1s1("MULT_S", PERIOD)
        value = payoff if value is None else value.v2s0("ADD", payoff)
        value = value.v2s1("DISCOUNT", L[p], OTHER_PERIOD) if kind == "other_period" else value.v2s0("MULT", L[p])
    return value.v1s1("FLOOR_S", 0.0).v2s0("DIV", numeraire)


def family_chain_oracle(o, kind, L, numeraire, periods, rate):
    from test_gpu_merged_chains import PERIOD, swaption_oracle
    if kind == "swaption":
        return swaption_oracle(o, L, numeraire, periods, rate)
    value = None
    for p in range(periods - 1, -1, -1):
        payoff = o.f_v1s1("MULT_S", o.f_v1s1("SUB_S", L[p], rate), PERIOD)
        value = payoff if value is None else o.f_v2s0("ADD", value, payoff)
        value = o.f_v2s1("DISCOUNT", value, L[p], OTHER_PERIOD) if kind == "other_period" else o.f_v2s0("MULT", value, L[p])
    return o.f_v2s0("DIV", o.f_v1s1("FLOOR_S", value, 0.0), numeraire)


class Family:
    """products: [(kind, periods, rate)] over `vectors` vectors drawn from `lo` … `hi`; merged: how many of them are chains of merged
    launches from the second round on; kernels: the family sizes whose merged kernels are recorded.  Shortest product first: the first
    `.moments()` runs everything pending with the moments taken along only when at least 256 methods are pending and four times as many
    as below the vector asked for (expectations_engine.hpp, Engine::reduce: BATCH_PENDING)."""

    def __init__(self, name, vectors, products, merged, kernels, lo=-0.01, hi=0.05):
        self.name, self.vectors, self.products, self.merged, self.kernels, self.lo, self.hi = name, vectors, products, merged, kernels, lo, hi

    def __repr__(self):
        return self.name


def _rates(tenors, kind="swaption", base=0.01):
    return [(kind, t, base + 0.002 * k) for k, t in enumerate(tenors)]


FAMILIES = [
    # merge_families: `if (fam.chain.size() == 16) { families.push_back(…); fam = Family(); }` … `if (fam.chain.size() >= 2) families.push_back(…)`:
    # the sixteen longest tenors are one family, the seventeenth is alone behind the split — no family — and runs as a launch of its own
    Family("seventeen_tenors", 44, _rates(range(12, 46, 2)), 16, (16,)),
    Family("two_tenors", 60, _rates((12, 60)), 2, (2,)),
    Family("one_tenor_discounts_with_another_period", 30, _rates((14, 18)) + [("other_period", 20, 0.02)] + _rates((24, 30), base=0.03), 4, (4,)),
    # two chains of every length ending in the same vector: the m-th chain of every length forms layer m, the layers are rows of one launch
    Family("two_layers", 30, _rates((14, 20, 30)) + _rates((14, 20, 30), base=0.02), 6, (3,)),
    Family("no_discount", 40, _rates((16, 24, 40), "no_discount", 0.9), 3, (3,), lo=0.9, hi=1.1),
]

# ------------------------------------------------------------------------------------------------ the catalogue
TWO_CARRIED = Shape("two_carried", two_carried_data, two_carried_device, two_carried_oracle, expect(4, inputs=2, carried=2, final=1, out=1),
                    plantable=("x", "y"))
FINAL_NOT_CARRIED = Shape("final_not_carried", final_not_carried_data, final_not_carried_device, final_not_carried_oracle,
                          expect(3, inputs=1, carried=1, final=2, out=1, peel=False), plantable=("x",))
MANY_IO = Shape("many_io", many_io_data, many_io_device, many_io_oracle, expect(6, globals=2, inputs=3, carried=1, final=1, out=3), plantable=("x", "y", "z", "g1"))
OPERAND_SLOTS_3 = Shape("operand_slots_3", operand_slots_data, _slots_device(SLOTS_3), _slots_oracle(SLOTS_3), expect(27, inputs=2, out=1), plantable=("x", "y"))
OPERAND_SLOTS_2 = Shape("operand_slots_2", operand_slots_data, _slots_device(SLOTS_2), _slots_oracle(SLOTS_2), expect(31, inputs=2, out=1), plantable=("x", "y"))
LIBRARY_MATH = Shape("library_math", library_math_data, library_math_device, library_math_oracle, expect(10, final=1, out=1, elems=4, peel=False), exact=False)
PEELED_LIBRARY = Shape("peeled_library_moments", peeled_library_data, peeled_library_device, peeled_library_oracle, expect(3, final=1, elems=4), exact=False)
LONG_HEAD_RELOAD = Shape("long_head_reload", long_head_data, long_head_device, long_head_oracle, expect(4, final=1))
ONE_MIDDLE_HANDLE = Shape("one_middle_handle", scan_data, _scan_device(11), _scan_oracle(11), expect(4, globals=1, out=2))
ALIASED = [Shape("aliased_two_iterations", aliased_a_data, _scan_device(None), _scan_oracle(None), None),
           Shape("aliased_both_slots", aliased_b_data, _scan_device(None), _scan_oracle(None), None),
           Shape("aliased_global_and_input", aliased_c_data, _scan_device(None), _scan_oracle(None), None)]

ROLLING = [TWO_CARRIED, FINAL_NOT_CARRIED, MANY_IO, OPERAND_SLOTS_3, OPERAND_SLOTS_2, LIBRARY_MATH, PEELED_LIBRARY, LONG_HEAD_RELOAD, ONE_MIDDLE_HANDLE] + LIMITS_INSIDE
EXACT = [s for s in ROLLING if s.exact] + ALIASED + LIMITS_OUTSIDE
PLANTED = [TWO_CARRIED, OPERAND_SLOTS_3, OPERAND_SLOTS_2, MANY_IO, FINAL_NOT_CARRIED]


# ------------------------------------------------------------------------------------------------ recorded descriptions
def parse_rolled(line):
    """One `rolled …` line of FMHIP_JIT_RECORD (jit.cpp: jit_describe(RolledBody)) → dict, None for any other line."""
    w = line.split()
    if not w or w[0] != "rolled":
        return None
    keys = ("elems", "log", "globals", "inputs", "carried", "final", "out", "body", "peel", "init", "preout", "postout", "finalstore", "pre", "post", "reduce", "chains", "sden")
    d, key = {}, None
    for t in w[1:]:
        if t in keys:
            key = t
            d[key] = []
        else:
            d[key].append(t)
    out = {k: int(d[k][0]) for k in ("elems", "log", "globals", "inputs")}
    out.update(period=len(d["body"]), carried=len(d["carried"]), final=len(d["final"]), out=len(d["out"]), peel="peel" in d, body=d["body"],
               reduce="reduce" in d, chains=int(d["chains"][0]) if "chains" in d else 0,
               pre=d.get("pre", []), post=d.get("post", []), preout=d.get("preout", []), postout=d.get("postout", []),
               finalstore=d.get("finalstore", []), final_pos=d["final"], carried_pos=d["carried"], extra=[int(x) for x in d.get("peel", [])], line=line)
    return out


def matches(desc, exp):
    return all(desc[k] == v for k, v in exp.items())


def expected_row_stores(desc):
    """{(word of the row, register array)} of every store a kernel makes through a pointer of its row's fixed part, from the row layout
    jit.cpp documents — plain: [G global][CI carried-in][CO final] …, peeled: [NX extra in][G global][CO final][NXO extra out] …: a plain
    kernel stores its final values (a carried one from its c register), a peeled one the stored values of its head and of its tail."""
    if not desc["peel"]:
        first = desc["globals"] + desc["carried"]
        return {(str(first + k), f"c{desc['carried_pos'].index(pos)}" if pos in desc["carried_pos"] else f"f{k}") for k, pos in enumerate(desc["final_pos"])}
    first = sum(desc["extra"]) + desc["globals"] + desc["final"]
    stores = {(str(first + k), "p" + i) for k, i in enumerate(desc["preout"])}
    stores |= {(str(first + len(desc["preout"]) + k), "q" + i) for k, i in enumerate(desc["postout"])}
    return stores                                 # (a peeled kernel stores no final value: the engine never sets Peel::final_store, see the module's text)
