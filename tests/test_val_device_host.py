"""CPU: device-resident validation without a GPU.  The new exports, the argument checks that run with a NULL handle, the
ground-truth half of the packing, and the NumPy statement of the append kernel (val_device_cases.append_rows) against
``val.convert_to_coco_format``, which test_host_logic pins to the reference on the same goldens."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, val
from lwpose_amd.runtime import Engine, coco_pack, coco_pack_gt

import coco_eval_cases as cc
import val_device_cases as vd

from conftest import ROOT

NEW_EXPORTS = ["lwp_coco_open", "lwp_coco_release", "lwp_coco_reset", "lwp_coco_add_maps", "lwp_coco_add_rows", "lwp_coco_counts",
               "lwp_coco_rows", "lwp_coco_finish", "lwp_debug_coco_rows"]


def last_error():
    return _lib.lib().lwp_last_error(None).decode()


def test_new_exports_are_declared_and_present():
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "lwpose.h")) as f:
        declared = set(re.findall(r"\b(lwp_[a-z_0-9]+)\s*\(", f.read()))
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name in declared, name
    assert L.lwp_version() >= 105


def open_store(p, row_cap=8, **override):
    q = dict(p, **override)
    rc = _lib.lib().lwp_coco_open(None, *Engine._coco_gt_args(q), row_cap)
    return rc, last_error()


def test_open_checks_the_ground_truth_as_coco_eval_does_without_a_handle():
    gt, dets, _ = cc.case("nd_chunk_minus_1")
    p = coco_pack_gt(gt)
    assert open_store(p) == (_lib.LWP_ERR_ARG, "handle is null")           # everything else passed
    assert open_store(p, n_images=0) == (_lib.LWP_ERR_ARG, "n_images must be at least 1")
    bad = p["gt_off"].copy(); bad[3] = bad[4] + 1
    assert open_store(p, gt_off=bad) == (_lib.LWP_ERR_ARG, "gt_off descends at image 3")
    bad = p["gt_off"].copy(); bad[0] = 1
    assert open_store(p, gt_off=bad)[1] == "gt_off[0] must be 0"
    for key, what in (("gt_kp", "ground-truth coordinate"), ("gt_area", "area"), ("gt_bbox", "box")):
        for v in (np.nan, np.inf, -np.inf):
            a = p[key].copy()
            a.reshape(-1)[-1] = v
            rc, msg = open_store(p, **{key: a})
            assert rc == _lib.LWP_ERR_ARG and what in msg and "not finite" in msg, (key, msg)
    rc, msg = open_store(p, row_cap=-1)
    assert rc == _lib.LWP_ERR_ARG and "row_cap" in msg
    L = _lib.lib()
    args = Engine._coco_gt_args(p)
    assert L.lwp_coco_open(None, args[0], None, *args[2:], 8) == _lib.LWP_ERR_ARG and last_error() == "gt_off is null"
    assert L.lwp_coco_open(None, *args[:2], None, *args[3:], 8) == _lib.LWP_ERR_ARG and "is null" in last_error()


def test_add_rows_and_the_read_outs_check_their_arguments_without_a_handle():
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    kp = np.ones((2, 17, 3))
    sc = np.array([0.5, 0.25])

    def add(kp, sc, n=2):
        return L.lwp_coco_add_rows(None, 0, n, kp.ctypes.data_as(dp) if kp is not None else None, sc.ctypes.data_as(dp) if sc is not None else None)
    assert add(kp, sc) == _lib.LWP_ERR_ARG and last_error() == "handle is null"
    assert add(kp, sc, n=-1) == _lib.LWP_ERR_ARG and "negative" in last_error()
    assert add(None, sc) == _lib.LWP_ERR_ARG and last_error() == "dt_kp / dt_score is null"
    assert add(kp, None) == _lib.LWP_ERR_ARG and last_error() == "dt_kp / dt_score is null"
    for v in (np.nan, np.inf, -np.inf):
        bad = kp.copy(); bad[1, 16, 1] = v
        assert add(bad, sc) == _lib.LWP_ERR_ARG and last_error() == "a detection coordinate is not finite"
        bad = sc.copy(); bad[1] = v
        assert add(kp, bad) == _lib.LWP_ERR_ARG and last_error() == "a detection score is not finite"
    z = np.zeros(3030)
    npig = np.zeros(3, dtype=np.int64)
    assert L.lwp_coco_finish(None, None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), npig.ctypes.data_as(C.POINTER(C.c_int64))) == _lib.LWP_ERR_ARG
    assert L.lwp_coco_finish(None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp),
                             npig.ctypes.data_as(C.POINTER(C.c_int64))) == _lib.LWP_ERR_ARG and last_error() == "handle is null"
    assert L.lwp_coco_counts(None, None, None) == _lib.LWP_ERR_ARG
    assert L.lwp_coco_rows(None, None, None, None, -1) == _lib.LWP_ERR_ARG
    assert L.lwp_coco_rows(None, None, None, None, 4) == _lib.LWP_ERR_ARG and "is null" in last_error()
    idx = (C.c_int * 1)(0)
    assert L.lwp_coco_add_maps(None, None, None, 0, 1, 4, 4, 4, 0, idx) == _lib.LWP_ERR_ARG
    assert L.lwp_debug_coco_rows(None, 0, None, None, None, None, None) == _lib.LWP_ERR_ARG
    for fn in (L.lwp_coco_release, L.lwp_coco_reset):
        assert fn(None) == _lib.LWP_ERR_ARG


@pytest.mark.parametrize("name", ["mixed", "nd1", "nd_chunk_plus_1"])
def test_pack_gt_is_the_ground_truth_half_of_pack(name):
    gt, dets, _ = cc.case(name)
    whole, half = coco_pack(gt, dets), coco_pack_gt(gt)
    assert sorted(half) == sorted(k for k in whole if not k.startswith("dt_"))
    assert sorted(whole) == sorted(["n_images", "image_ids", "dt_off", "dt_kp", "dt_score", "gt_off", "gt_kp", "gt_area", "gt_bbox",
                                    "gt_iscrowd", "gt_ignore"])
    for key, v in half.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == whole[key].dtype and v.shape == whole[key].shape and v.tobytes() == whole[key].tobytes(), key
        else:
            assert v == whole[key], key
    with pytest.raises(ValueError):
        coco_pack_gt(dict(gt, categories=[{"id": 1}, {"id": 2}]))


def test_the_numpy_statement_of_the_append_kernel_is_convert_to_coco_format():
    frames = vd.golden_frames()
    assert sum(len(e) for e, _ in frames.values()) >= 20
    batches = {k: v for k, v in vd.edge_batches().items()}
    for name, (entries, allk) in list(frames.items()) + [(b, f) for b, fs in batches.items() for f in fs]:
        kp, score = vd.append_rows(entries, allk)
        want_kp, want_score = val.convert_to_coco_format(entries, allk) if len(entries) else ([], [])
        assert kp.shape == (len(entries), 17, 3)
        assert kp.reshape(len(entries), 51).tolist() == [[float(v) for v in row] for row in want_kp], name
        assert score.tobytes() == np.array([float(s) for s in want_score], dtype=np.float64).tobytes(), name
    # the edge frames say what they are meant to say
    kp, score = vd.append_rows(*batches["count_one"][0])
    assert score.tolist() == [0.0, 0.0, 0.0] and np.signbit(score).tolist() == [False, True, False]
    kp, _ = vd.append_rows(*batches["neck_only"][0])
    assert not kp.any()
    kp, _ = vd.append_rows(*batches["one_keypoint_left"][0])
    assert (kp[0, :, 2] == 1).sum() == 1
    assert [len(f[0]) for f in batches["batch_2_0_5"]] == [2, 0, 5] and len(batches["full_frame"][0][0]) == 256


def test_evaluate_refuses_a_folder_and_visualize():
    with pytest.raises(TypeError, match="samples"):
        val.evaluate({}, None, "val2017/", None)
    with pytest.raises(NotImplementedError):
        val.evaluate({}, None, [], None, visualize=True)
