"""GPU: device-resident validation (lwp_coco_open .. lwp_coco_finish, coco_append_kernel / coco_gather_kernel in
csrc/eval_kernels.hip, val.evaluate).

Everything here is an equality.  The append kernel restates val.convert_to_coco_format with one float64 addition per
coordinate and one float64 multiplication per score, so its rows are compared bit for bit; the evaluation runs the kernels of
lwp_coco_eval on the same rows in the same order, so precision / recall / scores / npig are compared bit for bit with
``Engine.coco_eval``; val.evaluate is compared with ``coco_detections`` + ``evaluate_detections`` on the same samples."""
import ctypes
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth, val
from lwpose_amd._lib import CapacityError
from lwpose_amd.runtime import Engine, coco_pack, coco_pack_gt

import coco_eval_cases as cc
import val_device_cases as vd

pytestmark = pytest.mark.gpu

KEYS = ("precision", "recall", "scores", "npig", "stats")


@pytest.fixture(scope="module")
def eng():
    return Engine(0)


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return list(out)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def some_gt(n_images):
    """A ground truth of n_images images (ids 10, 20, ..), one person each."""
    anns = [cc.gt_ann(i + 1, 10 * (i + 1), cc.pose(200.0, 150.0, 80.0), 2500.0) for i in range(n_images)]
    return cc.dataset([10 * (i + 1) for i in range(n_images)], anns)


def pose_maps(seed, people=3):
    heat, paf, _ = synth.make_pose_maps(people, 46, 82, seed, 0.1, 0.02)
    return heat, paf


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ rows
def test_golden_frames_give_the_rows_of_convert_to_coco_format(eng):
    frames = {k: v for k, v in vd.golden_frames().items() if len(v[0])}
    names = sorted(frames)
    eng.coco_open(some_gt(len(names)))
    for i, name in enumerate(names):                   # one call per frame, in reverse image order
        eng.debug_coco_rows([frames[name]], [len(names) - 1 - i])
    rows = eng.coco_rows()
    at = 0
    for i, name in enumerate(reversed(names)):
        entries, allk = frames[name]
        want_kp, want_score = val.convert_to_coco_format(entries, allk)
        n = len(want_score)
        assert (rows["image"][at:at + n] == i).all()
        assert rows["keypoints"][at:at + n].reshape(n, 51).tolist() == [[float(v) for v in r] for r in want_kp], name
        assert same_bits(rows["score"][at:at + n], np.array([float(s) for s in want_score], dtype=np.float64)), name
        at += n
    assert at == len(rows["score"]) >= 20
    eng.coco_release()


@pytest.mark.parametrize("name", ["batch_2_0_5", "full_frame", "one_keypoint_left", "count_one", "neck_only"])
def test_edge_frames_bit_for_bit(eng, name):
    batch = vd.edge_batches(eng.caps[3])[name]
    eng.coco_open(some_gt(4), row_cap=sum(len(f[0]) for f in batch))       # exactly full
    index = [2, 0, 3][:len(batch)]
    eng.debug_coco_rows(batch, index)
    total, per = eng.coco_counts()
    assert total == sum(len(f[0]) for f in batch)
    assert per.tolist() == [len(batch[index.index(i)][0]) if i in index else 0 for i in range(4)]
    rows = eng.coco_rows()
    at = 0
    for i in sorted(index):                            # images ascending, entry order inside
        kp, score = vd.append_rows(*batch[index.index(i)])
        n = len(score)
        assert (rows["image"][at:at + n] == i).all()
        assert same_bits(rows["keypoints"][at:at + n], kp) and same_bits(rows["score"][at:at + n], score), i
        at += n
    assert at == total
    eng.coco_release()


# ------------------------------------------------------------------------------------------------ order
def test_rows_come_back_in_image_order_whatever_order_they_were_added_in(eng):
    maps = [pose_maps(s) for s in (2, 3, 4)]
    want = eng.poses_from_maps(np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps]), 4, False)
    assert all(len(w[0]) > 0 for w in want)
    eng.coco_open(some_gt(4))                          # image 3 is never added
    # frames 0, 1 as images [2, 0], then frame 2 as image [1]
    eng.coco_add_maps(cuda(np.stack([maps[0][0], maps[1][0]])), cuda(np.stack([maps[0][1], maps[1][1]])), [2, 0], 4, demo=False)
    eng.coco_add_maps(cuda(maps[2][0][None]), cuda(maps[2][1][None]), [1], 4, demo=False)
    with pytest.raises(RuntimeError, match="no pipeline run to fetch"):
        eng.fetch_poses()                              # the serial workspace holds nothing fetchable
    total, per = eng.coco_counts()
    frame_of = {2: 0, 0: 1, 1: 2}
    assert per.tolist() == [len(want[frame_of[i]][0]) for i in range(3)] + [0] and total == per.sum()
    rows = eng.coco_rows()
    at = 0
    for i in range(3):
        kp, score = vd.append_rows(want[frame_of[i]][0], want[frame_of[i]][1])
        n = len(score)
        assert (rows["image"][at:at + n] == i).all()
        assert same_bits(rows["keypoints"][at:at + n], kp) and same_bits(rows["score"][at:at + n], score), i
        at += n
    assert at == total
    eng.coco_release()


def test_rows_over_more_images_than_one_step_of_the_offset_scan(eng):
    """lwp_coco_rows forms dt_off on the device 256 images at a time (cc.SCAN_CHUNK): 2 * 256 + 1 images with 0 .. 3 rows each,
    added from the last image to the first, so that every source row moves."""
    n = 2 * cc.SCAN_CHUNK + 1
    r = np.random.RandomState(7)
    per = r.randint(0, 4, size=n)
    per[[cc.SCAN_CHUNK - 1, cc.SCAN_CHUNK, 2 * cc.SCAN_CHUNK]] = [1, 2, 3]
    kp = r.uniform(0.0, 500.0, size=(per.sum(), 17, 3))
    score = np.round(r.uniform(0.0, 1.0, size=per.sum()), 2)
    off = np.concatenate([[0], np.cumsum(per)])
    eng.coco_open(some_gt(n), row_cap=int(per.sum()))
    for i in reversed(range(n)):
        eng.coco_add_rows(i, kp[off[i]:off[i + 1]], score[off[i]:off[i + 1]])
    total, counts = eng.coco_counts()
    assert total == per.sum() and counts.tolist() == per.tolist()
    rows = eng.coco_rows()
    assert rows["image"].tolist() == np.repeat(np.arange(n), per).tolist()
    assert same_bits(rows["keypoints"], kp) and same_bits(rows["score"], score)
    eng.coco_release()


# ------------------------------------------------------------------------------------------------ evaluation
def push(eng, packed, seed):
    """The detections of a packed case through coco_add_rows, the images in a shuffled order."""
    order = np.random.RandomState(seed).permutation(packed["n_images"])
    for i in order:
        a, b = packed["dt_off"][i], packed["dt_off"][i + 1]
        eng.coco_add_rows(int(i), packed["dt_kp"][a:b], packed["dt_score"][a:b])


@pytest.mark.parametrize("name,build", [("mixed", cc.case_mixed), ("nd1", cc.case_nd1), ("total_small", lambda: cc.case_total(33, 300, small=True))])
def test_finish_equals_coco_eval_bit_for_bit(eng, name, build):
    gt, dets = build()
    packed = coco_pack(gt, dets)
    want = eng.coco_eval(packed)
    eng.coco_open(coco_pack_gt(gt), row_cap=len(dets))
    push(eng, packed, 1)
    got = eng.coco_finish()
    again = eng.coco_finish()                          # the store is left intact
    for key in KEYS:
        assert same_bits(got[key], want[key]) and same_bits(again[key], want[key]), (name, key)
    rows = eng.coco_rows()
    assert same_bits(rows["keypoints"], packed["dt_kp"]) and same_bits(rows["score"], packed["dt_score"])
    assert rows["image"].tolist() == np.repeat(np.arange(packed["n_images"]), np.diff(packed["dt_off"])).tolist()
    eng.coco_reset()                                   # the next validation of the same data set: another order, the same bits
    assert eng.coco_counts()[0] == 0
    push(eng, packed, 2)
    third = eng.coco_finish()
    for key in KEYS:
        assert same_bits(third[key], want[key]), (name, key)
    eng.coco_release()


def test_finish_then_more_rows_then_finish(eng):
    gt, dets = cc.case_mixed()
    packed = coco_pack(gt, dets)
    half = packed["n_images"] // 2
    part = [d for d in dets if packed["image_ids"].index(d["image_id"]) < half]
    eng.coco_open(gt)
    for i in range(packed["n_images"]):
        if i == half:
            first = eng.coco_finish()
            want = eng.coco_eval(gt, part)
            assert all(same_bits(first[k], want[k]) for k in KEYS)
        a, b = packed["dt_off"][i], packed["dt_off"][i + 1]
        eng.coco_add_rows(i, packed["dt_kp"][a:b], packed["dt_score"][a:b])
    got, want = eng.coco_finish(), eng.coco_eval(packed)
    assert all(same_bits(got[k], want[k]) for k in KEYS)
    eng.coco_release()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def net():
    from lwpose_amd import workload
    return workload.build_net(nref=1, seed=1, device=0, height=184, width=328, multiscale=[1])[0]


@pytest.fixture(scope="module")
def samples():
    """Four samples of two sizes, one of them blank; the ground truth lists a fifth image that has no sample."""
    out = [{"file_name": "%012d.jpg" % 785, "img": synth.make_frames(1, 184, 328, seed0=0)[0]},
           {"file_name": "%012d.jpg" % 139, "img": synth.make_frames(1, 160, 240, seed0=1)[0]},
           {"file_name": "%012d.jpg" % 4000, "img": np.full((184, 328, 3), 128, dtype=np.uint8)},
           {"file_name": "%012d.jpg" % 632, "img": synth.make_frames(1, 160, 240, seed0=2)[0]}]
    return out


def labels_for(results, extra_image):
    """Ground truth made of every second detection, shifted a little: AP and AR are fractions."""
    anns = []
    for n, r in enumerate(results[::2]):
        kp = np.array(r["keypoints"]).reshape(17, 3)
        vis = kp[:, 2] > 0
        xy = kp[vis, :2]
        w, h = np.ptp(xy[:, 0]), np.ptp(xy[:, 1])
        gkp = kp.copy()
        gkp[vis, :2] += 1.5
        gkp[vis, 2] = 2
        anns.append({"id": n + 1, "image_id": r["image_id"], "category_id": 1, "keypoints": gkp.reshape(-1).tolist(),
                     "num_keypoints": int(vis.sum()), "area": float(max(w * h, 1.0)), "iscrowd": 0,
                     "bbox": [float(xy[:, 0].min()), float(xy[:, 1].min()), float(w), float(h)]})
    return cc.dataset([785, 139, 4000, 632, extra_image], anns)


@pytest.mark.parametrize("multiscale", [False, True])
def test_evaluate_equals_the_dict_route(net, samples, tmp_path, multiscale):
    eng = net.engine
    results = val.coco_detections(net, samples, multiscale=multiscale, base_height=184)
    assert len(results) >= 2 and 4000 not in {r["image_id"] for r in results}
    gt = labels_for(results, 99999)
    with redirect_stdout(io.StringIO()) as ref_out:
        want_stats = val.evaluate_detections(gt, results, engine=eng)
    want = eng.coco_eval(gt, results)
    before = live()
    out = io.StringIO()
    with redirect_stdout(out):
        stats = val.evaluate(gt, str(tmp_path / "dt.json"), samples, net, multiscale=multiscale, store=True, base_height=184)
    with open(tmp_path / "dt.json") as f:
        written = json.load(f)
    assert written == results
    assert all(type(v) is float for r in written for v in r["keypoints"])
    assert same_bits(np.asarray(stats), np.asarray(want_stats)) and same_bits(np.asarray(stats), want["stats"])
    lines = out.getvalue().splitlines()
    assert lines[0] == "Running test for keypoints results." and lines[1:] == ref_out.getvalue().splitlines() and len(lines) == 11
    got = eng.coco_finish()                            # store=True: the store is still there, with this run's rows
    for key in KEYS:
        assert same_bits(got[key], want[key]), key
    # the next validation with the same labels reuses the resident ground truth; from a path and without a file it ends released
    with redirect_stdout(io.StringIO()):
        again = val.evaluate(gt, None, samples, net, multiscale=multiscale, store=True, base_height=184)
        with open(tmp_path / "gt.json", "w") as f:
            json.dump(gt, f)
        third = val.evaluate(str(tmp_path / "gt.json"), None, samples, net, multiscale=multiscale, base_height=184)
    assert same_bits(np.asarray(again), np.asarray(stats)) and same_bits(np.asarray(third), np.asarray(stats))
    assert live()[0] <= before[0]                      # released: no store, no ground truth left on the device
    with pytest.raises(RuntimeError, match="no detection store"):
        eng.coco_finish()
    with pytest.raises(ValueError, match="not in the ground truth"):
        with redirect_stdout(io.StringIO()):
            val.evaluate(gt, None, [{"file_name": "17.jpg", "img": samples[0]["img"]}], net, base_height=184)


# ------------------------------------------------------------------------------------------------ status
def test_a_frame_that_overflows_is_reported_by_every_read_out_until_reset():
    e2 = Engine(0)
    e2.set_capacity(64, 2, 16, 4)                      # what test_capacity_overflow_is_reported overflows with these maps
    heat, paf, _ = synth.make_pose_maps(5, 46, 82, 4, 0.15, 0.02)
    e2.coco_open(some_gt(4))
    blank = np.zeros_like(heat), np.zeros_like(paf)
    e2.coco_add_maps(cuda(np.stack([blank[0], heat])), cuda(np.stack([blank[1], paf])), [3, 2], 4, demo=True)
    for call in (e2.coco_finish, e2.coco_rows, e2.coco_counts, e2.coco_finish):
        with pytest.raises(CapacityError, match=r"image 2: post-processing capacity exceeded \(bits 0x[1-7]:"):
            call()
    e2.coco_reset()
    assert e2.coco_counts()[0] == 0
    e2.coco_add_maps(cuda(blank[0][None]), cuda(blank[1][None]), [2], 4, demo=True)      # image 2 may be added again
    assert e2.coco_finish()["npig"].tolist() == [4, 4, 0]
    e2.h.close()


def test_an_image_without_a_detection_may_be_the_first_add_after_open(eng):
    """n = 0 carries no host bytes: nothing of the (not yet allocated) pinned ring is touched, the image counts 0 rows, and the
    adds behind it work as ever.  Twice: every open starts without a ring."""
    b = cc.Builder(11)
    b.image(5, 2, 0)                                   # image 0 of the evaluation: people but no detection
    b.image(6, 1, 3)
    b.image(7, 0, 0)
    gt, dets = b.done()
    packed = coco_pack(gt, dets)
    assert np.diff(packed["dt_off"]).tolist() == [0, 3, 0]
    want = eng.coco_eval(packed)
    for _ in range(2):
        eng.coco_open(gt, row_cap=3)
        eng.coco_add_rows(0, np.zeros((0, 17, 3)), np.zeros(0))
        total, per = eng.coco_counts()
        assert total == 0 and per.tolist() == [0, 0, 0]
        first = eng.coco_finish()                      # nothing added yet but an empty image
        none = eng.coco_eval(gt, [])
        assert all(same_bits(first[k], none[k]) for k in KEYS)
        eng.coco_add_rows(2, np.zeros((0, 17, 3)), np.zeros(0))
        eng.coco_add_rows(1, packed["dt_kp"], packed["dt_score"])
        total, per = eng.coco_counts()
        assert total == 3 and per.tolist() == [0, 3, 0]
        got = eng.coco_finish()
        assert all(same_bits(got[k], want[k]) for k in KEYS)
        eng.coco_release()
    fresh = Engine(0)                                  # an engine that never opened a store: the library says so
    for call in (fresh.coco_counts, fresh.coco_rows, fresh.coco_finish):
        with pytest.raises(RuntimeError, match="no detection store"):
            call()
    fresh.h.close()


def test_unbound_ratio_and_non_finite_values_reach_the_status_word():
    e2 = Engine(0)
    heat, paf = pose_maps(2)
    nanpaf = np.full_like(paf, np.nan)                 # every mid-point fails before any passes: the reference's unbound 'ratio'
    with pytest.raises(UnboundLocalError):
        e2.poses_from_maps(heat[None], nanpaf[None], 4, False)       # what the fetch route reports for these maps
    e2.coco_open(some_gt(3))
    e2.coco_add_maps(cuda(heat[None]), cuda(paf[None]), [0], 4, demo=False)
    e2.coco_add_maps(cuda(heat[None]), cuda(nanpaf[None]), [2], 4, demo=False)
    for call in (e2.coco_counts, e2.coco_rows, e2.coco_finish):
        with pytest.raises(UnboundLocalError, match="'ratio' referenced before assignment"):
            call()
    e2.coco_reset()
    frame = vd.edge_batches()["one_keypoint_left"][0]
    k = frame[1].copy()
    k[7, 0] = np.inf                                   # the one key-point the pose refers to
    e2.debug_coco_rows([frame, (frame[0], k)], [0, 1])
    with pytest.raises(ValueError, match="image 1: a detection coordinate or score is not finite"):
        e2.coco_finish()
    e2.coco_reset()
    ent = frame[0].copy()
    ent[0, 18] = np.nan
    e2.debug_coco_rows([(ent, frame[1])], [2])
    with pytest.raises(ValueError, match="image 2: a detection coordinate or score is not finite"):
        e2.coco_rows()
    e2.coco_reset()
    e2.debug_coco_rows([frame], [2])
    assert e2.coco_counts()[0] == 1
    e2.h.close()


def test_row_cap_full_succeeds_and_one_short_names_the_count(eng):
    b = cc.Builder(9)
    b.image(1, 2, 5)
    b.image(2, 1, 3)
    gt, dets = b.done()
    packed = coco_pack(gt, dets)
    want = eng.coco_eval(packed)
    eng.coco_open(gt, row_cap=8)
    push(eng, packed, 0)
    got = eng.coco_finish()
    assert all(same_bits(got[k], want[k]) for k in KEYS) and eng.coco_counts()[0] == 8
    eng.coco_open(gt, row_cap=7)                       # a second open replaces the first
    push(eng, packed, 0)
    for call in (eng.coco_finish, eng.coco_rows):
        with pytest.raises(CapacityError, match="holds 7 rows and 8 were added .* row_cap >= 8"):
            call()
    eng.coco_reset()
    eng.coco_add_rows(1, packed["dt_kp"][5:8], packed["dt_score"][5:8])
    assert eng.coco_counts()[1].tolist() == [0, 3]
    eng.coco_open(gt, row_cap=0)
    assert eng.coco_finish()["npig"].tolist() == want["npig"].tolist()
    eng.coco_release()


def test_state_errors(eng):
    heat, paf = pose_maps(2)
    one = cuda(heat[None]), cuda(paf[None])
    eng.coco_release()
    for call in (eng.coco_finish, eng.coco_reset, lambda: eng.coco_add_rows(0, np.zeros((0, 17, 3)), np.zeros(0)),
                 lambda: eng.coco_add_maps(one[0], one[1], [0], 4)):
        with pytest.raises(RuntimeError, match="no detection store"):
            call()
    eng.coco_open(some_gt(2))
    eng.coco_add_maps(one[0], one[1], [1], 4)
    with pytest.raises(RuntimeError, match="image 1 was already added"):
        eng.coco_add_maps(one[0], one[1], [1], 4)
    with pytest.raises(RuntimeError, match="image 1 was already added"):
        eng.coco_add_rows(1, np.zeros((1, 17, 3)), np.zeros(1))
    with pytest.raises(RuntimeError, match="image 0 was already added"):
        eng.coco_add_maps(torch.cat([one[0]] * 2), torch.cat([one[1]] * 2), [0, 0], 4)
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="outside the ground truth"):
            eng.coco_add_maps(one[0], one[1], [bad], 4)
    n_before = eng.coco_counts()[0]
    eng.set_tracking(Engine.TRACK_LANES)
    with pytest.raises(RuntimeError, match="tracking is on"):
        eng.coco_add_maps(one[0], one[1], [0], 4)
    eng.set_tracking(0)
    assert eng.coco_counts()[0] == n_before            # nothing of the refused calls was enqueued
    eng.coco_release()
    e5 = Engine(0, num_heatmaps=6, num_pafs=8)
    import skeleton_cases as sc
    e5.set_skeleton(sc.GUIDE5_KPTS, sc.GUIDE5_PAFS, 5, 20)
    e5.coco_open(some_gt(2))
    with pytest.raises(RuntimeError, match="custom skeleton"):
        e5.coco_add_maps(cuda(np.zeros((1, 6, 8, 8), np.float32)), cuda(np.zeros((1, 8, 8, 8), np.float32)), [0], 4)
    e5.h.close()


# ------------------------------------------------------------------------------------------------ stream and lifetime
def test_add_on_the_callers_stream_is_seen_by_finish_and_everything_is_given_back():
    base = live()
    e2 = Engine(0)
    heat, paf = pose_maps(3)
    want = e2.poses_from_maps(heat[None], paf[None], 4, False)[0]
    side = torch.cuda.Stream()
    kp, score = vd.append_rows(want[0], want[1])
    assert len(score) > 0

    def cycle():
        before = live()
        e2.coco_open(some_gt(2))
        assert live()[0] > before[0]                   # the store and the ground truth are accounted for
        with torch.cuda.stream(side):                  # the maps are produced on the caller's stream, just before the call
            h = cuda(heat[None]) * 1.0
            p = cuda(paf[None]) * 1.0
            e2.coco_add_maps(h, p, [1], 4, demo=False)
            got = e2.coco_finish()                     # ordered behind the add: it sees the rows
            rows = e2.coco_rows()
        assert same_bits(rows["keypoints"], kp) and same_bits(rows["score"], score) and (rows["image"] == 1).all()
        assert got["npig"].tolist() == [2, 2, 0]
        e2.coco_release()
        e2.coco_release()                              # a second release is harmless

    cycle()                                            # whatever the first use keeps for good (the stream-ordering events) exists now
    started = live()
    cycle()
    assert live() == started                           # release gave back the store, the ground truth and the pinned ring
    e2.coco_open(some_gt(2))
    e2.h.close()                                       # destroy frees an open store too
    assert live() == base
