"""Custom skeletons, host side (no GPU): the oracle's grouping with patched tables reproduces the reference's own outputs
(tests/golden/skeleton_*.npz, tools/make_skeleton_golden.py), the regenerated inputs match the recorded digests, and the
drop-in group_keypoints refuses bad tables / sizes before it touches an engine."""
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd.modules import keypoints as kp_mod
from oracle import post_ref

import skeleton_cases as sc
from conftest import GOLDEN

MAP_NAMES = [c[0] for c in sc.MAP_CASES] + [c[0] for c in sc.OPTION_CASES]


def load(name):
    return np.load(os.path.join(GOLDEN, "skeleton_%s.npz" % name))


def up_maps(name, g):
    """(low-res heat, low-res paf, up-sampled heat HWC, up-sampled paf HWC) of a map case."""
    if name.startswith("coco_options"):
        heat, paf = sc.option_maps([c[1] for c in sc.OPTION_CASES if c[0] == name][0])
    else:
        heat, paf = sc.make_maps(sc.map_case(name))
    ratio = int(g["ratio"])
    return heat, paf, post_ref.upsample_cubic(heat.transpose(1, 2, 0), ratio), post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)


def oracle_post(monkeypatch, hu, pu, K, kpts, pafs, demo, E, mp):
    monkeypatch.setattr(post_ref, "KPT_IDS", [list(p) for p in kpts])
    monkeypatch.setattr(post_ref, "PAF_IDS", [list(p) for p in pafs])
    heat = hu.copy()
    by_type, total = [], 0
    for k in range(K):
        total += post_ref.extract_keypoints(heat[:, :, k], by_type, total)
    ent, allk = post_ref.group_keypoints(by_type, pu, pose_entry_size=E, min_paf_score=mp, demo=demo)
    return sc.flat_kp(by_type), np.asarray(ent, dtype=np.float64), np.asarray(allk, dtype=np.float64)


@pytest.mark.parametrize("name", MAP_NAMES)
def test_synth_digests_match(name):
    g = load(name)
    heat, paf, hu, pu = up_maps(name, g)
    assert str(g["lowres_digest"]) == sc.digest(heat) + sc.digest(paf)
    assert str(g["up_digest"]) == sc.digest(hu) + sc.digest(pu)


@pytest.mark.parametrize("name", MAP_NAMES)
def test_oracle_reproduces_skeleton_golden(monkeypatch, name):
    g = load(name)
    _, _, hu, pu = up_maps(name, g)
    K, E, mp = int(g["K"]), int(g["pose_entry_size"]), float(g["min_paf_score"])
    for tag, demo in (("demo", True), ("val", False)):
        kp, ent, allk = oracle_post(monkeypatch, hu, pu, K, g["limb_kpts"].tolist(), g["limb_pafs"].tolist(), demo, E, mp)
        assert np.array_equal(kp, g[tag + "_kp"]), tag
        assert tuple(ent.shape) == tuple(g[tag + "_entries_shape"]), tag
        assert np.array_equal(ent, g[tag + "_entries"]), tag
        assert np.array_equal(allk, g[tag + "_allk"]), tag


def test_oracle_reproduces_skeleton_adversarial_golden(monkeypatch):
    g = load("adversarial")
    cases = sc.adversarial_cases()
    assert sorted(cases) == sorted(k[3:] for k in g.files if k.startswith("kp:"))
    for name, (K, kpts, pafs, bt, paf) in cases.items():
        assert str(g["paf_digest:" + name]) == sc.digest(paf), name
        assert np.array_equal(sc.flat_kp(bt), g["kp:" + name]), name
        monkeypatch.setattr(post_ref, "KPT_IDS", kpts)
        monkeypatch.setattr(post_ref, "PAF_IDS", pafs)
        for tag, demo in (("demo", True), ("val", False)):
            ent, allk = post_ref.group_keypoints([list(l) for l in bt], paf, pose_entry_size=max(20, K + 2), demo=demo)
            key = "%s:%s" % (name, tag)
            assert tuple(np.asarray(ent).shape) == tuple(g["ent_shape:" + key]), key
            assert np.array_equal(np.asarray(ent, dtype=np.float64), g["ent:" + key]), key
            assert np.array_equal(np.asarray(allk, dtype=np.float64), g["allk:" + key]), key
    assert g["ent_shape:spill:demo"][0] > 64


class _NoEngine(object):
    """Any attribute access fails the test: the drop-in must refuse before it talks to an engine."""

    def __getattr__(self, name):
        raise AssertionError("engine touched (%s) before the argument checks" % name)


def _tables(monkeypatch, kpts, pafs):
    monkeypatch.setattr(kp_mod, "BODY_PARTS_KPT_IDS", kpts)
    monkeypatch.setattr(kp_mod, "BODY_PARTS_PAF_IDS", pafs)


def test_drop_in_refuses_small_pose_entry_size(monkeypatch):
    _tables(monkeypatch, sc.GUIDE5_KPTS, sc.GUIDE5_PAFS)
    with pytest.raises(ValueError, match="pose_entry_size"):
        kp_mod.group_keypoints([[] for _ in range(5)], np.zeros((8, 8, 8), np.float32), pose_entry_size=6, engine=_NoEngine())
    with pytest.raises(ValueError, match="pose_entry_size"):      # the COCO default needs 20: 19 would overwrite type 17
        _tables(monkeypatch, sc.COCO_KPTS, sc.COCO_PAFS)
        kp_mod.group_keypoints([[] for _ in range(18)], np.zeros((8, 8, 38), np.float32), pose_entry_size=19, engine=_NoEngine())


def test_drop_in_refuses_limb_ids_out_of_range(monkeypatch):
    _tables(monkeypatch, [[0, 1], [1, 5]], [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="limb 1"):
        kp_mod.group_keypoints([[] for _ in range(5)], np.zeros((8, 8, 4), np.float32), engine=_NoEngine())


def test_drop_in_refuses_limb_with_equal_ends(monkeypatch):
    _tables(monkeypatch, [[0, 1], [2, 2]], [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="limb 1"):
        kp_mod.group_keypoints([[] for _ in range(5)], np.zeros((8, 8, 4), np.float32), engine=_NoEngine())


def test_drop_in_reads_the_module_tables_at_call_time(monkeypatch):
    """The tables are looked up when group_keypoints runs (modules/keypoints.py:54-61), not bound at import."""
    _tables(monkeypatch, [[0, 1], [1, 7]], [[0, 1], [2, 3]])
    with pytest.raises(ValueError, match="limb 1"):
        kp_mod.group_keypoints([[] for _ in range(5)], np.zeros((8, 8, 4), np.float32), engine=_NoEngine())
    _tables(monkeypatch, [[0, 1], [1, 4]], [[0, 1], [2, 3]])
    with pytest.raises(AssertionError, match="engine touched"):     # valid now: the next step is the engine
        kp_mod.group_keypoints([[] for _ in range(5)], np.zeros((8, 8, 4), np.float32), engine=_NoEngine())
