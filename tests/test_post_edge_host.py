"""Edge cases of the post-processing chain, host side (no GPU): for every case of tests/post_edge_cases.py the rebuilt inputs
match the recorded digest, oracle/post_ref.py reproduces the reference's own output (tests/golden/post_edge_*.npz,
tools/make_post_edge_golden.py) bit for bit, and the oracle's counts show that the case sits on the boundary it names — so a
later edit to a builder cannot move a case off its boundary unnoticed."""
import os

import numpy as np
import pytest

import post_edge_cases as pc
from conftest import GOLDEN

CASES = pc.all_cases()
_G = {}


def golden(kind):
    if kind not in _G:
        _G[kind] = np.load(os.path.join(GOLDEN, "post_edge_%s.npz" % kind))
    return _G[kind]


def test_fixtures_hold_exactly_the_cases():
    for kind in ("group", "full", "maps"):
        have = sorted(k[len("digest:"):] for k in golden(kind).files if k.startswith("digest:"))
        assert have == sorted(n for n, c in CASES.items() if c["kind"] == kind)


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_reference_on_the_boundary(name):
    case = CASES[name]
    g = golden(case["kind"])
    assert str(g["digest:" + name]) == pc.input_digest(case)
    for tag, demo in (("demo", True), ("val", False)):
        key = "%s:%s" % (name, tag)
        if case["expect"].get("raises") == "unbound":
            assert int(g["unbound:" + key]) == 1
            with pytest.raises(UnboundLocalError):
                pc.run_oracle(case, demo)
            continue
        res = pc.run_oracle(case, demo)
        assert np.array_equal(res["kp"], g["kp:" + key]), key
        assert tuple(res["entries"].shape) == tuple(g["ent_shape:" + key]), key
        assert np.array_equal(res["entries"], g["ent:" + key]), key
        assert np.array_equal(res["allk"], g["allk:" + key]), key
        if case["kind"] == "full":
            assert np.array_equal(res["heat_mut"], g["mut:" + name], equal_nan=True), key
        if case["kind"] == "maps":
            assert pc.digest(res["heat_mut"]) == str(g["mut_digest:" + name]), key
        pc.check_expect(case, res)


def test_counts_parameter_changes_no_result():
    case = CASES["group/ties_60_of_100"]
    a = pc.run_oracle(case, True)
    b = pc.run_oracle(case, True, with_counts=False)
    assert np.array_equal(a["entries"], b["entries"]) and np.array_equal(a["allk"], b["allk"])
    assert a["counts"]["cand"][0] == 100 and b["counts"] is None


def test_named_switch_points_are_covered():
    """The boundary table of DESIGN.md section 4, as counts: each value must be some case's statement."""
    cand = {c["expect"].get("cand", {}).get(0) for c in CASES.values()}
    assert {64, 65, 1024, 1025, 4096} <= cand
    ents = {c["expect"].get("entries") for c in CASES.values()}
    assert {63, 64, 65} <= ents
    peaks = CASES["full/nms_counts"]["expect"]["peaks"]
    assert {63, 64, 65, 127, 128, 129, 256, 257} <= set(peaks.values())
    assert set(pc.PAIR_PRODUCTS.values()) == {1, 4, 5, 6, 19, 20, 21, 319, 320, 321}
    caps = [c["caps"]["max_entries"] for c in CASES.values() if c["caps"] and "max_entries" in c["caps"]]
    assert pc.ASSEMBLE_LDS_MAX_ENTRIES in caps and pc.ASSEMBLE_LDS_MAX_ENTRIES + 1 in caps
