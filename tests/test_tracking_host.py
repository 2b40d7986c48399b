"""Pose tail, host side (no GPU): the exports exist, their argument checks answer without a device, the Python tail
(demo.poses_from_entries + modules.pose.track_poses) reproduces the fixtures the device tail is tested against, and
run_demo refuses device_tail without fused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.modules import pose as pose_mod

import tracking_cases as tc
from conftest import ROOT

NEW_EXPORTS = ["lwp_set_tracking", "lwp_set_unmap", "lwp_reset_tracking", "lwp_get_poses", "lwp_track_poses",
               "lwp_debug_tracking_near"]


def test_exports_declared_and_present():
    header = open(os.path.join(ROOT, "include", "lwpose.h")).read()
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name


def _err():
    return _lib.lib().lwp_last_error(None).decode()


def test_argument_checks_need_no_gpu():
    L = _lib.lib()
    sig = (C.c_float * 5)(*([0.05] * 5))
    assert L.lwp_set_tracking(None, 4, 3, 0.5, 0, None, 0) == _lib.LWP_ERR_ARG and "mode" in _err()
    assert L.lwp_set_tracking(None, -1, 3, 0.5, 0, None, 0) == _lib.LWP_ERR_ARG and "mode" in _err()
    assert L.lwp_set_tracking(None, 2, 3, 0.5, 0, sig, 5) == _lib.LWP_ERR_ARG and "n_sigmas is 5" in _err()      # K is 18
    assert L.lwp_set_tracking(None, 2, 3, 0.5, 0, None, 5) == _lib.LWP_ERR_ARG and "sigmas is NULL" in _err()    # COCO table, not 18
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert L.lwp_set_tracking(None, 3, 3, bad, 0, None, 0) == _lib.LWP_ERR_ARG and "similarity_threshold" in _err()
    assert L.lwp_set_tracking(None, 2, 3, 0.5, 0, None, 18) == _lib.LWP_ERR_ARG and "handle" in _err()           # valid but no handle
    assert L.lwp_reset_tracking(None, -2, 0) == _lib.LWP_ERR_ARG and "lane" in _err()
    assert L.lwp_reset_tracking(None, 0, -1) == _lib.LWP_ERR_ARG and "next_id" in _err()
    assert L.lwp_track_poses(None, -1, 0, None, None, None, None, None, None, None) == _lib.LWP_ERR_ARG and "lane" in _err()
    assert L.lwp_set_unmap(None, 0, 1.0, 0, 0) == _lib.LWP_ERR_ARG and "stride" in _err()
    assert L.lwp_set_unmap(None, 8, 0.0, 0, 0) == _lib.LWP_ERR_ARG and "scale" in _err()


def _set_pose_tables(monkeypatch, K, sigmas, sim_threshold):
    monkeypatch.setattr(pose_mod.Pose, "num_kpts", K)
    monkeypatch.setattr(pose_mod.Pose, "sigmas", sigmas)
    monkeypatch.setattr(pose_mod.Pose, "vars", (sigmas * 2) ** 2)
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    monkeypatch.setattr(pose_mod._similar_keypoints, "__defaults__", (sim_threshold,))


@pytest.mark.parametrize("name", tc.tracking_case_names())
def test_python_tail_reproduces_tracking_fixture(monkeypatch, name):
    c = tc.tracking_case(name)
    _set_pose_tables(monkeypatch, c["K"], c["sigmas"], c["similarity_threshold"])
    prev = []
    inherited = 0
    for fr in c["frames"]:
        cur = [pose_mod.Pose(kp.copy(), float(cf)) for kp, cf in zip(fr["in_kp"], fr["in_conf"])]
        before = set(p.id for p in prev)
        with np.errstate(over="ignore"):
            pose_mod.track_poses(prev, cur, threshold=c["match_threshold"], smooth=c["smooth"])
        assert [p.id for p in cur] == fr["out_ids"].tolist()
        assert np.array_equal(np.stack([p.keypoints for p in cur]), fr["out_kp"])
        assert np.array_equal(np.array([p.bbox for p in cur], np.int32).reshape(-1, 4), fr["out_bbox"])
        assert pose_mod.Pose.last_id == fr["last_id"]
        inherited += sum(1 for p in cur if p.id in before)
        prev = cur
    assert (inherited > 0) == (c["match_threshold"] <= c["K"])


@pytest.mark.parametrize("name", tc.unmap_case_names())
def test_python_tail_reproduces_unmap_fixture(name):
    c = tc.unmap_case(name)
    poses = demo.poses_from_entries(c["entries"], c["all_keypoints"], c["scale"], c["pad"], c["stride"], c["ratio"])
    assert np.array_equal(np.stack([p.keypoints for p in poses]), c["out_kp"])
    assert np.array_equal(np.array([p.confidence for p in poses]), c["out_conf"])
    assert np.array_equal(np.array([p.bbox for p in poses], np.int32).reshape(-1, 4), c["out_bbox"])


def test_poses_from_arrays_matches_pose_objects():
    c = tc.unmap_case("demo_like")
    poses = pose_mod.poses_from_arrays(c["out_kp"], c["out_conf"], c["out_bbox"], np.arange(len(c["out_conf"]), dtype=np.int32))
    for i, p in enumerate(poses):
        assert np.array_equal(p.keypoints, c["out_kp"][i]) and p.keypoints.dtype == np.int32
        assert p.bbox == tuple(int(v) for v in c["out_bbox"][i]) == pose_mod.Pose.get_bbox(c["out_kp"][i])
        assert p.confidence == c["out_conf"][i] and p.id == i and p.filters is None


class _Engine(object):
    skeleton = {"num_kpt_types": 18}

    def __getattr__(self, name):
        raise AssertionError("engine touched (%s) before the argument checks" % name)


class _Net(object):
    engine = _Engine()


def test_run_demo_device_tail_needs_fused():
    with pytest.raises(ValueError, match="fused=True"):
        demo.run_demo(_Net(), [], 256, False, True, True, fused=False, device_tail=True)


def test_run_demo_custom_skeleton_needs_device_tail_and_sigmas():
    class E5(_Engine):
        skeleton = {"num_kpt_types": 5}

    class N5(object):
        engine = E5()
    with pytest.raises(ValueError, match="key-point types"):
        demo.run_demo(N5(), [], 256, False, True, True, fused=True)
    with pytest.raises(ValueError, match="key-point types"):
        demo.run_demo(N5(), [], 256, False, True, True, fused=True, device_tail=True)                 # no sigmas
    with pytest.raises(ValueError, match="key-point types"):
        demo.run_demo(N5(), [], 256, False, True, True, fused=True, device_tail=True, sigmas=[.05] * 5, draw=True)
