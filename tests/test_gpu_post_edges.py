"""Edge cases of the post-processing chain on the GPU (-m gpu): every case of tests/post_edge_cases.py through the entry point
it names and the drop-in modules.keypoints functions, on the specialised COCO kernels and on the generic ones
(LWP_POST_GENERIC=1), against the reference's own output (tests/golden/post_edge_*.npz).  Every comparison is bit-exact, and
Engine.post_counts must equal the oracle's counts: together with the case's boundary statement (checked on the CPU by
tests/test_post_edge_host.py) that shows the intended form of each kernel ran.  "Must raise" cases are error codes of the
library, never faults."""
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd._lib import CapacityError
from lwpose_amd.modules import keypoints as kp_mod
from lwpose_amd.runtime import Engine

import post_edge_cases as pc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()
_G, _ENG, _ORA = {}, {}, {}


def golden(kind):
    if kind not in _G:
        _G[kind] = np.load(os.path.join(GOLDEN, "post_edge_%s.npz" % kind))
    return _G[kind]


def engine(generic=False, tile=None, caps=None):
    """An Engine created under LWP_POST_GENERIC / LWP_PEAK_TILE (both are read at creation); cached unless it has capacities of
    its own."""
    key = (generic, tile)
    if caps is None and key in _ENG:
        return _ENG[key]
    env = {"LWP_POST_GENERIC": "1" if generic else None, "LWP_PEAK_TILE": None if tile is None else str(tile)}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        e = Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert e.post_generic == generic
    if caps is not None:
        e.set_capacity(**caps)
    else:
        _ENG[key] = e
    return e


def oracle(name, demo):
    if (name, demo) not in _ORA:
        _ORA[name, demo] = pc.run_oracle(CASES[name], demo)
    return _ORA[name, demo]


def counts_of(kp):
    return np.bincount(kp[:, 4].astype(int), minlength=18) if len(kp) else np.zeros(18, int)


def check_counts(eng, frame, ora, peaks=True):
    got_peaks, got_kpts, got_cand, got_picked = eng.post_counts(frame)
    c = ora["counts"]
    if peaks:
        assert got_peaks.tolist() == c["peaks"], (got_peaks.tolist(), c["peaks"])
    assert got_kpts.tolist() == c["kpts"], (got_kpts.tolist(), c["kpts"])
    assert got_cand.tolist() == c["cand"], (got_cand.tolist(), c["cand"])
    assert got_picked.tolist() == c["picked"], (got_picked.tolist(), c["picked"])


# ------------------------------------------------------------------------------------------------ "group" cases
GROUP = sorted(n for n, c in CASES.items() if c["kind"] == "group")


@pytest.mark.parametrize("generic", [False, True], ids=["coco", "generic"])
@pytest.mark.parametrize("name", GROUP)
def test_group_case(name, generic):
    case = CASES[name]
    g = golden("group")
    eng = engine(generic, caps=case["caps"])
    kp = pc.flat_kp(case["by_type"])
    raises = case["expect"].get("raises")
    for tag, demo in (("demo", True), ("val", False)):
        key = "%s:%s" % (name, tag)
        if raises:
            err = CapacityError if raises == "capacity" else UnboundLocalError
            with pytest.raises(err):
                eng.group_keypoints(kp[:, :4], counts_of(kp), case["paf"], demo)
            with pytest.raises(err):
                kp_mod.group_keypoints([list(l) for l in case["by_type"]], case["paf"], demo=demo, engine=eng)
            continue
        ora = oracle(name, demo)
        want = g["ent:" + key]
        ent = eng.group_keypoints(kp[:, :4], counts_of(kp), case["paf"], demo)
        assert ent.shape == want.reshape(-1, 20).shape, (key, ent.shape)
        assert np.array_equal(ent, want.reshape(-1, 20)), key
        check_counts(eng, 0, ora, peaks=False)
        d_ent, d_allk = kp_mod.group_keypoints([list(l) for l in case["by_type"]], case["paf"], demo=demo, engine=eng)
        assert tuple(np.asarray(d_ent).shape) == tuple(g["ent_shape:" + key]), key
        assert np.array_equal(np.asarray(d_ent, dtype=np.float64), want), key
        assert np.array_equal(np.asarray(d_allk, dtype=np.float64), g["allk:" + key]), key
        assert eng.post_generic == generic                       # the drop-in pushed no other skeleton


# ------------------------------------------------------------------------------------------------ "full" and "maps" cases
MAPS = sorted(n for n, c in CASES.items() if c["kind"] in ("full", "maps"))
# (generic kernels, LWP_PEAK_TILE): every tile geometry on the COCO kernels (the column form exists for ratio 4 and 8 only: at
# ratio 1 the launcher maps 4 to tile 3, and the result must be the same), the default choice on both
VARIANTS = [(False, None), (True, None)] + [(False, t) for t in range(5)]


def run_maps(eng, case, heat3, paf3, demo, batch):
    """The case's frame alone (batch False), or as frame 1 of a batch of three whose other frames are other maps."""
    if case["kind"] == "full":
        args = dict(upsample_ratio=1, demo=demo, layout="NHWC")
    else:
        args = dict(upsample_ratio=case["ratio"], demo=demo)
    if batch:
        return eng.poses_from_maps(heat3, paf3, **args)[1]
    return eng.poses_from_maps(heat3[1:2], paf3[1:2], **args)[0]


@pytest.mark.parametrize("generic,tile", VARIANTS, ids=["coco", "generic"] + ["tile%d" % t for t in range(5)])
@pytest.mark.parametrize("name", MAPS)
def test_maps_case(name, generic, tile):
    case = CASES[name]
    g = golden(case["kind"])
    eng = engine(generic, tile, caps=case["caps"])
    others = pc.other_frames(case)
    heat3 = np.stack([others[0], case["heat"], others[1]])
    paf = case["paf"] if case["kind"] == "maps" else np.zeros(case["heat"].shape[:2] + (38,), np.float32)
    paf3 = np.stack([paf, paf, paf])
    raises = case["expect"].get("raises")
    for tag, demo in (("demo", True), ("val", False)):
        key = "%s:%s" % (name, tag)
        if raises:
            with pytest.raises(CapacityError):
                run_maps(eng, case, heat3, paf3, demo, False)
            with pytest.raises(CapacityError, match="frame 1"):
                run_maps(eng, case, heat3, paf3, demo, True)
            continue
        ora = oracle(name, demo)
        gk = g["kp:" + key]
        for frame in (0, 1):
            ent, allk, counts = run_maps(eng, case, heat3, paf3, demo, frame == 1)
            assert np.array_equal(allk, g["allk:" + key].reshape(-1, 4)), (key, frame)
            assert np.array_equal(counts, counts_of(gk)), (key, frame)
            assert ent.shape == g["ent:" + key].reshape(-1, 20).shape, (key, frame, ent.shape)
            assert np.array_equal(ent, g["ent:" + key].reshape(-1, 20)), (key, frame)
            check_counts(eng, frame, ora)


@pytest.mark.parametrize("tile", [None, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["kind"] == "full"))
def test_full_case_through_drop_in_extract(name, tile):
    """modules.keypoints.extract_keypoints per channel view (find_peaks_kernel<1, ..> + nms_kernel on one map): the key-point
    tuples and the heat map it thresholds in place."""
    case = CASES[name]
    g = golden("full")
    eng = engine(False, tile, caps=case["caps"])
    heat = case["heat"].copy()
    if case["expect"].get("raises"):
        with pytest.raises(CapacityError):
            for k in range(18):
                kp_mod.extract_keypoints(heat[:, :, k], [], 0, engine=eng)
        return
    bt, total = [], 0
    for k in range(18):
        total += kp_mod.extract_keypoints(heat[:, :, k], bt, total, engine=eng)
    assert np.array_equal(pc.flat_kp(bt), g["kp:%s:demo" % name])
    assert np.array_equal(heat, g["mut:" + name], equal_nan=True)


def test_in_place_nhwc_view_of_the_network_path():
    pytest.skip("LWP_POST_NCHW=0 makes the grouping read the network's NHWC concat buffer in place; only infer_poses reaches it, "
                "and no entry point can feed that buffer hand-made maps (poses_from_maps copies its maps to planes)")
