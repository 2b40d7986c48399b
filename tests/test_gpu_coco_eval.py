"""GPU: COCO key-point evaluation (lwp_coco_eval / lwp_debug_coco_oks, csrc/eval_kernels.hip) against the NumPy restatement of
COCOeval in coco_eval_cases.py.  The case builders assert that no OKS entry lies within 1e-9 of a threshold and that no two
candidates of a detection tie by less, so the discrete results cannot depend on the last bits of exp(): the selected order, the
matched / ignored bits and npig must be identical, precision / recall / scores bit for bit (integer counts, IEEE divisions),
the ten stats within 1e-12.  The OKS entries themselves: 17 terms in [0, 1], each with a few roundings in e and one exp of at
most 1 ulp, then the sum and the division, stay under 32 * 2^-53 of the restatement's; the bar is twice that, 2^-47 absolute.

Shapes (coco_eval_cases.CASES): "mixed" holds an image with detections but no ground truth, one with ground truths but no
detection and one with neither; D = 1, 20, 21, 45; G = 1, 33, 65, 130; crowds, people without and with some hidden key-points;
areas 1024 and 9216; score ties across images; an identical detection.  The data-set sizes 1, 255, 256, 257 and 589 sit around
the accumulate kernel's scan step of 256 (SCAN_CHUNK); "nd1" and "nd_chunk_plus_1" hold ranges without a counted ground truth."""
import ctypes
import json

import numpy as np
import pytest
import torch  # noqa: F401

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth, val
from lwpose_amd.runtime import Engine, coco_pack

import coco_eval_cases as cc

pytestmark = pytest.mark.gpu

OKS_BAR = 2.0 ** -47


@pytest.fixture(scope="module")
def eng():
    return Engine(0)


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return list(out)


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", list(cc.CASES))
def test_accumulated_arrays_are_bit_equal_to_the_restatement(eng, name):
    gt, dets, ref = cc.case(name)
    packed = coco_pack(gt, dets)
    eng.coco_eval(packed)                              # whatever the first call of a process allocates for good is there now
    before = live()
    got = eng.coco_eval(packed)
    again = eng.coco_eval(gt, dets)
    assert live() == before
    for key in ("precision", "recall", "scores", "npig", "stats"):
        assert same_bits(got[key], again[key]), key
    assert got["npig"].tolist() == ref.npig.tolist()
    assert same_bits(got["precision"], np.ascontiguousarray(ref.eval["precision"][:, :, 0, :, 0]))
    assert same_bits(got["recall"], np.ascontiguousarray(ref.eval["recall"][:, 0, :, 0]))
    assert same_bits(got["scores"], np.ascontiguousarray(ref.eval["scores"][:, :, 0, :, 0]))
    np.testing.assert_allclose(got["stats"], ref.stats, rtol=0, atol=1e-12)
    assert ((got["stats"] == -1) == (ref.stats == -1)).all()


@pytest.mark.parametrize("name", ["mixed", "nd1", "nd_chunk_plus_1"])
def test_per_image_results_against_the_restatement(eng, name):
    gt, dets, ref = cc.case(name)
    packed = coco_pack(gt, dets)
    eng.debug_coco_oks(packed, image=0)
    before = live()
    worst = 0.0
    for i in range(packed["n_images"]):
        want = cc.image_reference(ref, i)
        got = eng.debug_coco_oks(packed, image=i)
        again = eng.debug_coco_oks(gt, dets, image=i)
        assert got["order"] == again["order"] and same_bits(got["oks"], again["oks"])
        assert same_bits(got["matched"], again["matched"]) and same_bits(got["ignored"], again["ignored"])
        assert got["order"] == want["order"], i
        assert got["npig"].tolist() == want["npig"].tolist(), i
        assert got["oks"].shape == want["oks"].shape, i
        if want["oks"].size:
            worst = max(worst, float(np.max(np.abs(got["oks"] - want["oks"]))))
        assert (got["matched"] == want["matched"]).all(), i
        assert (got["ignored"] == want["ignored"]).all(), i
    assert live() == before
    print("worst OKS difference in %s: %.3e (bar %.3e)" % (name, worst, OKS_BAR))
    assert worst <= OKS_BAR
    if name == "mixed":                                # the identical detection of image 3: OKS exactly 1, matched at 0.95
        i = packed["image_ids"].index(3)
        got = eng.debug_coco_oks(packed, image=i)
        assert got["oks"].tolist() == [[1.0]] and got["matched"][0, 9, 0]


def test_run_coco_eval_on_files(eng, tmp_path, capsys):
    gt, dets, ref = cc.case("nd_chunk")
    with open(tmp_path / "gt.json", "w") as f:
        json.dump(gt, f)
    with open(tmp_path / "dt.json", "w") as f:
        json.dump(dets, f)
    want = eng.coco_eval(gt, dets)["stats"]
    capsys.readouterr()
    got = val.run_coco_eval(str(tmp_path / "gt.json"), str(tmp_path / "dt.json"))
    lines = capsys.readouterr().out.splitlines()
    assert same_bits(np.asarray(got), want)
    assert lines[0] == "Running test for keypoints results." and lines[1:] == ref.lines and len(lines) == 11
    with pytest.raises(ValueError):
        val.evaluate_detections(gt, dets + [dict(dets[0], image_id=123456789)])


def test_end_to_end_detections_scored_against_themselves():
    """val.coco_detections on a synthetic-weights net, then evaluate_detections against ground truth made of its own detections:
    every person is found exactly, AP and AR are 1 in 'all'."""
    from lwpose_amd import workload
    net, _ = workload.build_net(nref=1, seed=1, device=0, height=184, width=328, multiscale=[1])
    samples = [{"file_name": "%012d.jpg" % (139 + 7 * i), "img": synth.make_frames(1, 184, 328, seed0=i)[0]} for i in range(2)]
    results = val.coco_detections(net, samples, multiscale=False, base_height=184)
    assert len(results) >= 2
    anns = []
    for n, r in enumerate(results):
        kp = np.array(r["keypoints"]).reshape(17, 3)
        vis = kp[:, 2] > 0
        xy = kp[vis, :2]
        w, h = np.ptp(xy[:, 0]), np.ptp(xy[:, 1])
        gkp = kp.copy()
        gkp[vis, 2] = 2
        anns.append({"id": n + 1, "image_id": r["image_id"], "category_id": 1, "keypoints": gkp.reshape(-1).tolist(),
                     "num_keypoints": int(vis.sum()), "area": float(max(w * h, 1.0)), "iscrowd": 0,
                     "bbox": [float(xy[:, 0].min()), float(xy[:, 1].min()), float(w), float(h)]})
    gt = cc.dataset(sorted({r["image_id"] for r in results}), anns)
    stats = val.evaluate_detections(gt, results, engine=net.engine)
    np.testing.assert_allclose(stats[[0, 1, 2]], 1.0, rtol=0, atol=4e-16)      # an AP of one is 1 - 2^-52 (tp / (tp + fp + 2^-52))
    assert stats[5] == 1 and stats[6] == 1 and stats[7] == 1
