"""CPU: COCO key-point evaluation without a GPU.  The NumPy restatement of COCOeval (coco_eval_cases.CocoEvalRef) is pinned to
closed-form cases that need no library; the packing of the data sets, the ten stats and the argument checks of the two C
entry points are tested where they need no device."""
import ctypes as C

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine, coco_pack, coco_stats

import coco_eval_cases as cc


def stats_of(gt, dets):
    return cc.reference(gt, dets).stats


def close(got, want):
    """An AP of "1" is tp / (tp + fp + 2^-52) = 1 - 2^-52 in floating point, in pycocotools as here: two units in the last place."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert ((got == -1) == (want == -1)).all(), got
    np.testing.assert_allclose(got, want, rtol=0, atol=4e-16)


def one_person(area, image_id=1, ann_id=1, at=(200.0, 150.0)):
    xy = cc.pose(at[0], at[1], 80.0)
    return xy, cc.gt_ann(ann_id, image_id, xy, area)


# ------------------------------------------------------------------------------------------------ closed-form cases
@pytest.mark.parametrize("area,want", [(2500.0, [1, 1, 1, 1, -1, 1, 1, 1, 1, -1]), (20000.0, [1, 1, 1, -1, 1, 1, 1, 1, -1, 1])])
def test_one_person_found_exactly(area, want):
    xy, a = one_person(area)
    close(stats_of(cc.dataset([1], [a]), [cc.det(1, xy, 0.9)]), want)


def test_two_people_one_found():
    """recall stops at 0.5: precision is 1 at the 51 recall thresholds up to 0.5 and 0 beyond, AP = 51/101."""
    xy, a = one_person(2500.0)
    _, b = one_person(2500.0, ann_id=2, at=(450.0, 300.0))
    s = stats_of(cc.dataset([1], [a, b]), [cc.det(1, xy, 0.9)])
    close(s, [51.0 / 101.0] * 4 + [-1] + [0.5] * 4 + [-1])


def test_a_far_detection_ahead_of_the_right_one():
    """precision after the false positive at 0.9 and the match at 0.5 is 1/2 at every recall threshold."""
    xy, a = one_person(2500.0)
    s = stats_of(cc.dataset([1], [a]), [cc.det(1, cc.far_pose(), 0.9), cc.det(1, xy, 0.5)])
    close(s, [0.5] * 4 + [-1] + [1] * 4 + [-1])


def test_crowd_ground_truths_match_repeatedly_and_their_matches_are_ignored():
    xy, a = one_person(2500.0)
    cxy = cc.pose(450.0, 300.0, 80.0)
    crowd = cc.gt_ann(2, 1, cxy, 2500.0, iscrowd=1)
    dets = [cc.det(1, xy, 0.9), cc.det(1, cxy, 0.8), cc.det(1, cxy + 0.25, 0.7)]
    ref = cc.reference(cc.dataset([1], [a, crowd]), dets)
    close(ref.stats, [1, 1, 1, 1, -1, 1, 1, 1, 1, -1])
    e = ref.evalImgs[0]
    assert (e["dtMatches"][0] == [1, 2, 2]).all() and (e["dtIgnore"][0] == [False, True, True]).all()


def test_areas_on_a_range_edge_count_on_both_sides():
    xy, a = one_person(1024.0)
    xy2, b = one_person(9216.0, ann_id=2, at=(450.0, 300.0))
    ref = cc.reference(cc.dataset([1], [a, b]), [cc.det(1, xy, 0.9), cc.det(1, xy2, 0.8)])
    assert ref.npig.tolist() == [2, 2, 1]              # all; medium holds both edges; large holds 9216
    assert ref.stats[5] == 1 and ref.stats[8] == 1 and ref.stats[9] == 1


def test_the_21st_detection_is_dropped_and_the_earlier_of_a_tie_survives():
    xy, a = one_person(2500.0)
    far = cc.far_pose()
    # 19 far detections at 0.9, then two at 0.5: the far one comes first and takes rank 19, the right one is the 21st
    dets = [cc.det(1, far + i, 0.9) for i in range(19)] + [cc.det(1, far, 0.5), cc.det(1, xy, 0.5)]
    ref = cc.reference(cc.dataset([1], [a]), dets)
    assert len(ref.evalImgs[0]["dtScores"]) == 20 and ref.stats[0] == 0 and ref.stats[5] == 0
    assert cc.image_reference(ref, 0)["order"] == list(range(20))
    # with the two swapped the right one survives
    dets[19], dets[20] = dets[20], dets[19]
    ref = cc.reference(cc.dataset([1], [a]), dets)
    assert ref.stats[5] == 1 and ref.stats[0] == pytest.approx(1.0 / 20.0, abs=1e-15)


def test_every_case_meets_the_builders_conditions():
    for name in cc.CASES:
        gt, dets, ref = cc.case(name)
        assert cc.check_conditions(ref) >= 1e-9
    total = {name: len(cc.case(name)[1]) for name in cc.CASES}
    assert [total[k] for k in ("nd1", "nd_chunk_minus_1", "nd_chunk", "nd_chunk_plus_1", "nd_beyond_two_chunks")] == \
        [1, cc.SCAN_CHUNK - 1, cc.SCAN_CHUNK, cc.SCAN_CHUNK + 1, 2 * cc.SCAN_CHUNK + 77]
    ref = cc.case("nd_chunk_plus_1")[2]
    assert ref.npig[1] == 0 and ref.stats[3] == -1     # a range without a counted ground truth


# ------------------------------------------------------------------------------------------------ packing and stats
def test_pack_orders_images_by_id_and_keeps_input_order_within_one():
    gt, dets, ref = cc.case("mixed")
    p = coco_pack(gt, dets)
    ids = ref.params.imgIds
    assert p["image_ids"] == ids and p["n_images"] == len(ids)
    for i, img in enumerate(ids):
        want_d = [d["score"] for d in dets if d["image_id"] == img]
        assert p["dt_score"][p["dt_off"][i]:p["dt_off"][i + 1]].tolist() == want_d
        want_g = [a["area"] for a in gt["annotations"] if a["image_id"] == img]
        assert p["gt_area"][p["gt_off"][i]:p["gt_off"][i + 1]].tolist() == want_g
    flat = [g for img in ids for g in ref._gts[img, 1]]
    assert p["gt_ignore"].tolist() == [int(bool(g["ignore"])) for g in flat]
    assert p["gt_kp"].shape == (len(flat), 17, 3) and p["dt_kp"].shape == (len(dets), 17, 3)


def test_pack_refuses_what_the_evaluation_does_not_support():
    xy, a = one_person(2500.0)
    gt = cc.dataset([1], [a])
    with pytest.raises(ValueError):
        coco_pack(gt, [cc.det(2, xy, 0.5)])            # loadRes asserts this
    with pytest.raises(ValueError):
        coco_pack(cc.dataset([1], [dict(a, id=0)]), [])
    with pytest.raises(ValueError):
        coco_pack(dict(gt, categories=[{"id": 1}, {"id": 2}]), [])


def test_stats_are_the_means_of_summarize():
    for name in ("mixed", "nd_chunk_plus_1"):
        ref = cc.case(name)[2]
        got = coco_stats(ref.eval["precision"][:, :, 0, :, 0], ref.eval["recall"][:, 0, :, 0])
        assert got.tolist() == ref.stats.tolist()


def test_summary_lines_have_cocoevals_format(capsys):
    from lwpose_amd.val import _print_summary
    ref = cc.case("mixed")[2]
    _print_summary(ref.stats)
    assert capsys.readouterr().out.splitlines() == ref.lines
    assert ref.lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = %0.3f" % ref.stats[0]


# ------------------------------------------------------------------------------------------------ the C entry points
def call_eval(p, **override):
    L = _lib.lib()
    q = dict(p, **override)
    out = [np.zeros(3030), np.zeros(30), np.zeros(3030), np.zeros(3, dtype=np.int64)]
    dp = C.POINTER(C.c_double)
    rc = L.lwp_coco_eval(None, *Engine._coco_args(q), out[0].ctypes.data_as(dp), out[1].ctypes.data_as(dp), out[2].ctypes.data_as(dp),
                         out[3].ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, L.lwp_last_error(None).decode()


def test_new_exports_and_version():
    L = _lib.lib()
    for name in ("lwp_coco_eval", "lwp_debug_coco_oks"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lwp_version() >= 104


def test_argument_checks_need_no_gpu():
    gt, dets, _ = cc.case("nd_chunk_minus_1")
    p = coco_pack(gt, dets)
    rc, msg = call_eval(p)
    assert rc == _lib.LWP_ERR_ARG and "handle" in msg  # everything else passed
    bad_off = p["dt_off"].copy(); bad_off[3] = bad_off[4] + 1
    assert call_eval(p, dt_off=bad_off) == (_lib.LWP_ERR_ARG, "dt_off descends at image 3")
    bad_off = p["gt_off"].copy(); bad_off[0] = 1
    assert call_eval(p, gt_off=bad_off)[1] == "gt_off[0] must be 0"
    assert call_eval(p, n_images=0)[0] == _lib.LWP_ERR_ARG
    for key, what in (("dt_score", "score"), ("dt_kp", "detection coordinate"), ("gt_kp", "ground-truth coordinate"),
                      ("gt_area", "area"), ("gt_bbox", "box")):
        for v in (np.nan, np.inf, -np.inf):
            a = p[key].copy()
            a.reshape(-1)[-1] = v
            rc, msg = call_eval(p, **{key: a})
            assert rc == _lib.LWP_ERR_ARG and what in msg and "not finite" in msg, (key, msg)
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    args = Engine._coco_args(p)
    z = np.zeros(3030)
    assert L.lwp_coco_eval(None, *args, None, z.ctypes.data_as(dp), z.ctypes.data_as(dp), None) == _lib.LWP_ERR_ARG
    assert L.lwp_coco_eval(None, args[0], None, *args[2:], z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp),
                           np.zeros(3, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))) == _lib.LWP_ERR_ARG
    # the debug twin: the same checks, then its own
    n_sel, order, npig = C.c_int(), (C.c_int * 20)(), (C.c_int * 3)()
    m = (C.c_ubyte * 600)()
    oks = np.zeros(4)
    assert L.lwp_debug_coco_oks(None, *args, 0, None, order, oks.ctypes.data_as(dp), 4, m, m, npig) == _lib.LWP_ERR_ARG
    assert L.lwp_debug_coco_oks(None, *args, p["n_images"], C.byref(n_sel), order, oks.ctypes.data_as(dp), 4, m, m, npig) == _lib.LWP_ERR_ARG
    img = int(np.argmax(np.diff(p["gt_off"]) * np.minimum(np.diff(p["dt_off"]), 20)))
    assert L.lwp_debug_coco_oks(None, *args, img, C.byref(n_sel), order, oks.ctypes.data_as(dp), 1, m, m, npig) == _lib.LWP_ERR_CAPACITY
