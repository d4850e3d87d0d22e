"""The producing side passes back to back on ONE engine (csrc/side_pass_engine.hpp: they share the pinned stage, the other scratch, the flag's
sequence and — through Engine::PassOutputs — the way their outputs become vectors): polynomial and binned evaluation, sort by key, rank
scores, prefix sums, tabulated functions, named functions, option formulas, block moments (small blocks and one block of the whole sample)
and the repeat, through the C-ABI, in two different orders with reducing passes and host-result calls between them.  Every result must
equal, BIT FOR BIT, the result of the same call made alone right after a fresh fmhip_init — no tolerance: a call that read a neighbour's
table, flag or buffer differs.  What the calls compute is checked by each pass's own GPU test; this one checks that they do not meet.

Sizes: one element; 2049, just past one 2048-element segment of the block moments and one tile of the prefix pass; 65537.  The engine is
shut down and initialised again and again, so everything runs in ONE child process and the tests read what it printed."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 2049, 65537]
SMALL_BLOCK = {1: 1, 2049: 3, 65537: 1}             # divisors of the size (65537 is prime); the large block is the whole sample
CALLS = ["polynomial_evaluate", "binned_evaluate", "sort_by_key", "rank_scores", "prefix_sums", "table_apply", "function_apply", "option_formula",
         "block_moments", "block_moments_whole", "repeat"]
ORDERS = {"forward": CALLS, "shuffled": ["repeat", "table_apply", "block_moments_whole", "sort_by_key", "option_formula", "polynomial_evaluate", "prefix_sums",
                                         "block_moments", "function_apply", "rank_scores", "binned_evaluate"]}


def case(n):
    """Six columns: a key with NaN, ±inf and -0.0 among its elements from 8 on, two regressors, a probability, a forward and a volatility."""
    import numpy as np
    rng = np.random.default_rng(7000 + n)
    key = rng.standard_normal(n).astype(np.float32)
    if n >= 8: key[:4] = [np.nan, np.inf, -np.inf, -0.0]
    return {"key": key, "x0": rng.standard_normal(n).astype(np.float32), "x1": rng.standard_normal(n).astype(np.float32),
            "u": rng.uniform(0.01, 0.99, n).astype(np.float32), "forward": rng.uniform(0.5, 1.5, n).astype(np.float32),
            "vol": rng.uniform(0.1, 0.4, n).astype(np.float32)}


def producing_calls(fm, n, v):
    """name → a function that makes the call on the uploaded columns `v` and returns its new vectors as DeviceVectors."""
    import ctypes as C
    import numpy as np
    lib, check, DV = fm.lib(), fm._native.check, fm.DeviceVector
    i64s = lambda hs: (C.c_int64 * len(hs))(*hs)
    dbls = lambda a: (C.c_double * len(a))(*[float(x) for x in a])
    h = {k: dv.handle for k, dv in v.items()}

    def made(out, size):
        return [DV(int(x), size) for x in out]

    def polynomial_evaluate():
        out = i64s([0])
        e = (C.c_uint8 * 6)(0, 0, 1, 2, 3, 0)
        check(lib.fmhip_polynomial_evaluate(i64s([h["x0"], h["x1"]]), 2, e, 3, i64s([h["u"], 0]), 2, dbls([0.5, -1.25, 0.125, 2.0, 3.0]), out))
        return made(out, n)

    def binned_evaluate():
        out = i64s([0])
        check(lib.fmhip_binned_evaluate(h["key"], dbls([-0.5, 0.0, 0.7]), 4, i64s([0, h["x0"]]), 2, dbls([1.0, 2.0, -1.0, 0.5, 3.0, -2.0, 0.25, 1.0]), out))
        return made(out, n)

    def sort_by_key():
        key_out, values_out = i64s([0]), i64s([0, 0])
        check(lib.fmhip_sort_by_key(h["key"], i64s([h["x0"], h["u"]]), 2, key_out, values_out))
        return made(key_out, n) + made(values_out, n)

    def rank_scores():
        out = i64s([0])
        check(lib.fmhip_rank_scores(h["x1"], out))
        return made(out, n)

    def prefix_sums():
        out, total = i64s([0]), C.c_double(0.0)
        check(lib.fmhip_prefix_sums(h["u"], 1, out, C.byref(total)))
        return made(out, n) + [np.array([total.value])]

    def table_apply():
        knots, count = np.linspace(-2.0, 2.0, 9), 9
        coefficients = (C.c_double * (2 * (count + 1) * 4))()
        for t, (values, interpolation, extrapolation) in enumerate(((np.sin(knots), 2, 1), (knots ** 2, 1, 0))):
            part = (C.c_double * ((count + 1) * 4))()
            check(lib.fmhip_table_build(dbls(knots), dbls(values), count, interpolation, extrapolation, 0, part))
            coefficients[t * (count + 1) * 4:(t + 1) * (count + 1) * 4] = part[:]
        out = i64s([0, 0])
        check(lib.fmhip_table_apply(h["x0"], dbls(knots), count, coefficients, 2, out))
        return made(out, n)

    def function_apply():
        out = i64s([0, 0, 0])
        check(lib.fmhip_function_apply(h["u"], (C.c_int * 3)(2, 0, 1), 3, out))
        return made(out, n)

    def option_formula():
        out = i64s([0, 0, 0])
        check(lib.fmhip_option_formula(0, h["forward"], 0.0, h["vol"], 0.0, 0, 1.0, 2.0, 1.0, 7, out))
        return made(out, n)

    def block_moments_of(block):
        def call():
            out = i64s([0] * 6)
            check(lib.fmhip_block_moments(i64s([h["x0"], h["forward"]]), 2, block, 7, out))
            return made(out, n // block)
        return call

    def repeat():
        out = i64s([0])
        check(lib.fmhip_vec_repeat(h["x1"], 2, 3, out))
        return made(out, 6 * n)

    return {"polynomial_evaluate": polynomial_evaluate, "binned_evaluate": binned_evaluate, "sort_by_key": sort_by_key, "rank_scores": rank_scores,
            "prefix_sums": prefix_sums, "table_apply": table_apply, "function_apply": function_apply, "option_formula": option_formula,
            "block_moments": block_moments_of(SMALL_BLOCK[n]), "block_moments_whole": block_moments_of(n), "repeat": repeat}


def between(fm, n, v, k):
    """The k-th thing between two producing calls: a reducing pass or a host-result call that uses the same stage, scratch and flag."""
    import numpy as np
    which = k % 5
    if which == 0: fm.cross_moments([None, v["x0"], v["x1"]], [v["u"]])
    elif which == 1: fm.binned_cross_moments(v["key"], [-0.5, 0.0, 0.7], [None, v["x0"]], [v["x1"]])
    elif which == 2: v["x0"].count_not_above([-0.5, 0.0, np.inf])
    elif which == 3: fm.prefix_sums_at(v["u"], [0, n - 1])
    else: fm.read_elements(v["x1"], [n - 1, 0])


def digest(results):
    import hashlib
    import numpy as np
    return [hashlib.sha1((r if isinstance(r, np.ndarray) else r.to_float32()).tobytes()).hexdigest() for r in results]


def run_all(fm):
    """{size: {"alone": {call: digests}, order: {call: digests}}}: every init … shutdown holds its vectors in a scope of its own."""
    def fresh(n, names, with_between):
        fm.init(0)
        out = {}
        try:
            def body():
                v = {k: fm.DeviceVector.from_host(a) for k, a in case(n).items()}
                calls = producing_calls(fm, n, v)
                for k, name in enumerate(names):
                    out[name] = digest(calls[name]())
                    if with_between: between(fm, n, v, k)
            body()
        finally:
            fm.purge()
            fm.shutdown()
        return out

    res = {}
    for n in SIZES:
        res[str(n)] = {"alone": {name: fresh(n, [name], False)[name] for name in CALLS}}
        for order, names in ORDERS.items():
            res[str(n)][order] = fresh(n, names, True)
    return res


_CHILD = r'''
import importlib, json, sys
sys.path[:0] = [%(root)r, %(tests)r]
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
from test_gpu_producing_pass_sequence import run_all
print("RESULT " + json.dumps(run_all(fm)))
'''


@pytest.fixture(scope="module")
def results(gpu, tmp_path_factory):
    script = tmp_path_factory.mktemp("producing") / "sequence.py"
    script.write_text(_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("n", SIZES)
def test_back_to_back_equals_alone_bit_for_bit(results, n, order):
    alone, together = results[str(n)]["alone"], results[str(n)][order]
    assert sorted(together) == sorted(CALLS) == sorted(alone)
    different = [name for name in CALLS if together[name] != alone[name]]
    assert not different, (n, order, different)


def test_the_sequence_is_a_test(results):
    """The digests tell results apart: different calls and different sizes give different bits, and every call made a vector."""
    for n in SIZES:
        alone = results[str(n)]["alone"]
        assert all(len(alone[name]) >= 1 for name in CALLS)
        assert alone["table_apply"][0] != alone["table_apply"][1] and alone["rank_scores"] != alone["repeat"]
    assert results["2049"]["alone"]["prefix_sums"] != results["65537"]["alone"]["prefix_sums"]
