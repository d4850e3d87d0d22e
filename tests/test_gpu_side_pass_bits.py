"""The bits of the fp64 sums of the reducing side passes — rank sums, cross moments, binned cross moments, kernel moments, wide and polynomial
cross moments — against tests/golden/side_pass_bits.json, recorded from the commit that file names by tests/golden/make_side_pass_bits.py
(the cases, the inputs and the sizes are its: one ragged workgroup, one full, two, 65, and a workgroup that takes two tiles; one and many
slices along gridDim.y).  The passes' own tests hold the sums to derived error bounds, which any order of the additions satisfies; this one
pins the order itself — the tree of csrc/side_pass_device.hpp and of the kernels in front of it."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_side_pass_bits", os.path.join(GOLDEN, "make_side_pass_bits.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

CASES = recorder.cases()
FIXTURE = json.load(open(recorder.FIXTURE))


def test_the_fixture_holds_every_case():
    assert sorted(FIXTURE["cases"]) == sorted(c["id"] for c in CASES)
    assert len(FIXTURE["commit"]) == 40


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_bits(gpu, case):
    want = FIXTURE["cases"][case["id"]]
    got = recorder.run(gpu, case)
    have = recorder.digest(got)
    differing = [i for i, (a, b) in enumerate(zip(have["first"], want["first"])) if a != b]
    print(f"{case['id']}: {got.size} values, sha256 {have['sha256'][:16]} (recorded {want['sha256'][:16]}), of the first {len(want['first'])} values {len(differing)} differ")
    assert have["first"] == want["first"], (case["id"], differing, [have["first"][i] for i in differing], [want["first"][i] for i in differing])
    assert have["sha256"] == want["sha256"], case["id"]
    assert np.isfinite(got).all()
