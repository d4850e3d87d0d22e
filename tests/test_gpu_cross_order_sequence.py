"""The order statistics across vectors and the selection behind their index BETWEEN the other producing side passes on ONE engine
(csrc/side_pass_engine.hpp; the frame of tests/test_gpu_producing_pass_sequence.py, whose columns, calls and digests this file uses): sort
by key, then the two new passes, then the block moments and the named functions, with reducing passes and host-result calls between them.
Every result must equal, BIT FOR BIT, the result of the same call made alone right after a fresh fmhip_init — a call that read a
neighbour's table, flag or buffer differs.  What the calls compute is checked by tests/test_gpu_cross_order.py; this one checks that they do
not meet.  The engine is shut down and initialised again and again, so everything runs in ONE child process."""
import json
import os
import subprocess
import sys

import pytest

from test_gpu_producing_pass_sequence import SIZES, between, case, digest, producing_calls

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQUENCE = ["sort_by_key", "cross_order", "cross_order_values", "cross_select", "block_moments", "function_apply"]


def calls_with_cross_order(fm, n, v):
    import ctypes as C
    lib, check, DV = fm.lib(), fm._native.check, fm.DeviceVector
    calls = producing_calls(fm, n, v)
    five = (C.c_int64 * 5)(v["key"].handle, v["x0"].handle, v["x1"].handle, v["u"].handle, v["x0"].handle)

    def cross_order():
        out = (C.c_int64 * 6)()
        check(lib.fmhip_cross_order_statistics(five, 5, (C.c_int32 * 3)(4, 0, 2), 3, 3, out))
        return [DV(int(x), n) for x in out]

    def cross_order_values():
        out = (C.c_int64 * 2)()
        check(lib.fmhip_cross_order_statistics(five, 3, (C.c_int32 * 2)(2, 2), 2, 1, out))
        return [DV(int(x), n) for x in out]

    def cross_select():
        slot = (C.c_int64 * 1)()
        check(lib.fmhip_cross_order_statistics(five, 5, (C.c_int32 * 1)(3), 1, 2, slot))
        index = DV(int(slot[0]), n)
        out = (C.c_int64 * 1)()
        check(lib.fmhip_cross_select(index.handle, five, 5, out))
        return [index, DV(int(out[0]), n)]

    calls.update({"cross_order": cross_order, "cross_order_values": cross_order_values, "cross_select": cross_select})
    return calls


def run_all(fm):
    def fresh(n, names, with_between):
        fm.init(0)
        out = {}
        try:
            def body():
                v = {k: fm.DeviceVector.from_host(a) for k, a in case(n).items()}
                calls = calls_with_cross_order(fm, n, v)
                for k, name in enumerate(names):
                    out[name] = digest(calls[name]())
                    if with_between: between(fm, n, v, k)
            body()
        finally:
            fm.purge()
            fm.shutdown()
        return out
    return {str(n): {"alone": {name: fresh(n, [name], False)[name] for name in SEQUENCE}, "together": fresh(n, SEQUENCE, True)} for n in SIZES}


_CHILD = r'''
import importlib, json, sys
sys.path[:0] = [%(root)r, %(tests)r]
fm = importlib.import_module("finmath-lib-cuda-extensions_amd")
from test_gpu_cross_order_sequence import run_all
print("RESULT " + json.dumps(run_all(fm)))
'''


@pytest.fixture(scope="module")
def results(gpu, tmp_path_factory):
    script = tmp_path_factory.mktemp("cross_order") / "sequence.py"
    script.write_text(_CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("n", SIZES)
def test_between_the_other_passes_equals_alone_bit_for_bit(results, n):
    alone, together = results[str(n)]["alone"], results[str(n)]["together"]
    assert sorted(together) == sorted(SEQUENCE) == sorted(alone)
    different = [name for name in SEQUENCE if together[name] != alone[name]]
    assert not different, (n, different)
    assert len(alone["cross_order"]) == 6
    if n > 1: assert len(set(alone["cross_order"][:3])) == 3                                  # the digests tell the ranks apart
    assert alone["cross_order_values"][0] == alone["cross_order_values"][1]                  # a duplicate selector: the same bits twice
