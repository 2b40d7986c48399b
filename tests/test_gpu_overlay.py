"""Pose overlay on the GPU (-m gpu): the kernels through Engine.draw_poses at the smallest shapes where each thing can go wrong,
then through the one-call video step, run_demo and run_cameras.  Every comparison is exact; the expected frames come from the
NumPy reference of tests/overlay_cases.py, which tests/test_overlay_host.py holds against the host rasteriser Pose.draw."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import overlay_cases as oc
import skeleton_cases as sc
import video_cases as vc

pytestmark = pytest.mark.gpu

DRAWN = oc.COCO_LIMBS[:-2]


@pytest.fixture(scope="module")
def eng():
    return Engine(0)


@pytest.fixture(scope="module")
def net():
    n = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(n, {"state_dict": vc.state_dict()})
    return n.eval().cuda(0)


def expected(frames, kps, limbs=DRAWN, **kw):
    return np.stack([oc.render(f, k, oc.bbox_of(k), limbs, **kw) for f, k in zip(frames, kps)])


# ------------------------------------------------------------------------------------------ 1. the kernels through draw_poses
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", oc.EDGE_SHAPES)
def test_edge_poses_on_host_and_device_memory(eng, H, W, N):
    frames = oc.noise_frames(N, H, W, seed=H + N)
    kps = oc.batch_poses(N, H, W)
    want = expected(frames, kps)
    assert (want != frames).any() and tuple(want[-1, 0, 0]) == oc.BOX_COLOR       # the empty pose's box paints pixel (0, 0)
    boxes = [oc.bbox_of(k) for k in kps]
    keep = frames.copy()
    got = eng.draw_poses(frames, kps, boxes)                                      # host -> host
    assert isinstance(got, np.ndarray) and np.array_equal(got, want) and np.array_equal(frames, keep)
    d = torch.from_numpy(frames).cuda(0)
    got_d = eng.draw_poses(d, kps, boxes)                                         # device -> device
    assert got_d.is_cuda and np.array_equal(got_d.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), keep)
    assert np.array_equal(eng.draw_poses(d, kps, boxes, device_out=False), want)  # device -> host
    assert np.array_equal(eng.draw_poses(frames, kps, boxes, device_out=True).cpu().numpy(), want)   # host -> device
    if N == 1:                                                                    # one frame (H,W,3), and a source off the 16-byte grid
        assert np.array_equal(eng.draw_poses(frames[0], kps[0], boxes[0]), want[0])
        flat = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda:0")
        flat[1:] = d.reshape(-1)
        assert np.array_equal(eng.draw_poses(flat[1:].reshape(1, H, W, 3), kps, boxes).cpu().numpy(), want)


def test_padded_arrays_with_pose_counts(eng):
    H, W = 37, 53
    frames = oc.noise_frames(3, H, W, seed=5)
    kps = oc.batch_poses(3, H, W)
    kp = np.full((3, 7, 18, 2), 9, np.int32)             # the slots beyond a frame's count hold key-points that must not be drawn
    bb = np.full((3, 7, 4), 3, np.int32)
    for f, k in enumerate(kps):
        kp[f, :len(k)] = k
        bb[f, :len(k)] = oc.bbox_of(k)
    got = eng.draw_poses(frames, kp, bb, n_poses=[len(k) for k in kps])
    assert np.array_equal(got, expected(frames, kps))


def test_step_loop_beyond_one_wave(eng):
    frames = oc.noise_frames(1, 200, 320, seed=7)
    kps = [oc.long_limb_poses()]
    assert abs(kps[0][0, 4] - kps[0][0, 3]).max() > 256 and abs(kps[0][0, 7] - kps[0][0, 6]).max() > 64
    assert np.array_equal(eng.draw_poses(frames, kps, [oc.bbox_of(kps[0])]), expected(frames, kps))


def test_256_poses_in_one_frame(eng):
    frames = oc.noise_frames(1, 16, 16, seed=8)
    kps = [oc.crowd256()]
    want = expected(frames, kps)
    assert np.array_equal(eng.draw_poses(frames, kps, [oc.bbox_of(kps[0])]), want)
    want = expected(frames, kps, boxes=False)
    assert (want == frames).all(axis=-1).any()           # part of the frame stays unpainted
    eng.set_overlay(0, boxes=False)
    try:
        assert np.array_equal(eng.draw_poses(frames, kps, [oc.bbox_of(kps[0])]), want)
    finally:
        eng.set_overlay(0)


def test_far_outside_end_points(eng):
    frames = oc.noise_frames(1, 24, 40, seed=9)
    kps = [oc.far_poses()]
    want = expected(frames, kps)
    assert (want != frames).any()
    assert np.array_equal(eng.draw_poses(frames, kps, [oc.bbox_of(kps[0])]), want)
    # rows saturated at int32: the call completes, and no stamp reaches a pixel more than a few steps off the diagonal x == y
    sat = oc.saturated_poses()
    box = np.array([[oc.INT32_MIN, oc.INT32_MIN, 0, 0]], np.int32)               # what the tail's wrapping box arithmetic gives
    got = eng.draw_poses(frames, [sat], [box])
    yy, xx = np.mgrid[0:24, 0:40]
    off = np.abs(xx - yy) > 4
    assert np.array_equal(got[0][off], frames[0][off])


def test_colours_boxes_and_drawn_limbs(eng):
    H, W = 37, 53
    frames = oc.noise_frames(1, H, W, seed=11)
    full = oc.edge_poses(H, W)
    full[0, [0, 1, 2, 5]] = [(20, 5), (22, 12), (15, 14), (30, 14)]               # head and shoulders: limbs 0, 1 and the last two exist
    kps, boxes = [full], [oc.bbox_of(full)]
    try:
        for nd in (0, 1, 19):
            eng.set_overlay(0, color=(200, 10, 77), box_color=(1, 2, 3), n_draw_limbs=nd)
            want = expected(frames, kps, oc.COCO_LIMBS[:nd], color=(200, 10, 77), box_color=(1, 2, 3))
            assert np.array_equal(eng.draw_poses(frames, kps, boxes), want), nd
        assert not np.array_equal(expected(frames, kps, oc.COCO_LIMBS), expected(frames, kps))    # the last two limbs paint something
        eng.set_overlay(0, boxes=False, n_draw_limbs=0)
        assert np.array_equal(eng.draw_poses(frames, kps, boxes), frames)         # nothing drawn: the plain copy
        with pytest.raises(ValueError, match="n_draw_limbs"):
            eng.set_overlay(0, n_draw_limbs=20)
    finally:
        eng.set_overlay(0)
    assert np.array_equal(eng.draw_poses(frames, kps, boxes), expected(frames, kps))


def test_custom_skeleton_reads_the_engines_limb_table():
    e = Engine(0, num_heatmaps=22, num_pafs=40)
    e.set_skeleton(sc.HAND21_KPTS, sc.HAND21_PAFS, 21)
    rs = np.random.RandomState(21)
    kp = rs.randint(-4, 60, (3, 21, 2)).astype(np.int32)
    kp[rs.rand(3, 21) < 0.2] = -1
    frames = oc.noise_frames(1, 48, 56, seed=12)
    want = expected(frames, [kp], sc.HAND21_KPTS[:-2])
    assert np.array_equal(e.draw_poses(frames, [kp], [oc.bbox_of(kp)]), want)
    assert not np.array_equal(want, expected(frames, [kp], sc.HAND21_KPTS))


# ------------------------------------------------------------------------------------------ 2. through the video step
def submit_fetch(e, frames, slot):
    e.pipeline_submit_u8(frames, slot, 368)
    res = e.pipeline_fetch(slot)
    return res, e.poses(slot)


def check_slot(e, slot, frames, rows):
    got = e.pipeline_overlay(slot)
    want = np.stack([oc.render(f, r["keypoints"], r["bbox"], DRAWN) for f, r in zip(frames, rows)])
    assert np.array_equal(got, want)
    assert np.array_equal(e.pipeline_overlay(slot, device=True).cpu().numpy(), want)
    return sum(len(r["ids"]) for r in rows), int((want != np.asarray(frames)).any(axis=-1).sum())


@pytest.mark.parametrize("mode,smooth,ov_mode", [(Engine.TRACK_LANES, False, 2), (Engine.TRACK_SEQUENCE, True, 2), (Engine.TRACK_LANES, False, 1)])
def test_pipeline_overlay_equals_render_of_the_slots_own_rows(net, mode, smooth, ov_mode):
    e = net.engine
    frames = np.stack(vc.pipe_frames("480x640", 4))
    e.set_tracking(mode, smooth=smooth)
    e.set_overlay(ov_mode)
    try:
        poses = painted = 0
        for slot, batch in ((0, frames[:1]), (1, frames[1:4]), (0, frames[:3])):   # batch 1, batch 3, and frames seen before (smoothing)
            _, rows = submit_fetch(e, batch, slot)
            n, px = check_slot(e, slot, batch, rows)
            poses += n
            painted += px
        assert poses >= 2 and painted > 0
        d = torch.from_numpy(frames[:1]).cuda(0)                                   # device frames are read in place
        _, rows = submit_fetch(e, d, 1)
        check_slot(e, 1, frames[:1], rows)
    finally:
        e.set_overlay(0)
        e.set_tracking(0)


def test_each_slot_owns_its_frames(net):
    e = net.engine
    a = np.stack(vc.pipe_frames("480x640", 1))
    b = np.stack(vc.pipe_frames("720x1280", 1, seed0=3))
    a_keep = a.copy()
    e.set_tracking(Engine.TRACK_ROWS)
    e.set_overlay(2)
    try:
        e.pipeline_submit_u8(a, 0, 368)
        a[:] = 255 - a                                   # host frames are free on return
        e.pipeline_submit_u8(b, 1, 368)                  # another size: the shared upload staging would be reallocated and overwritten
        e.pipeline_fetch(0)
        e.pipeline_fetch(1)
        ra, rb = e.poses(0), e.poses(1)
        na, pa = check_slot(e, 0, a_keep, ra)
        nb, pb = check_slot(e, 1, b, rb)
        assert na >= 1 and nb >= 1 and pa > 0 and pb > 0
        with pytest.raises(ValueError, match="annotated frames of 480 x 640"):
            _lib.check(_lib.lib().lwp_get_overlay(e.h.ptr, 0, a.ctypes.data, 0, 1, 480, 641), e.h.ptr)
    finally:
        e.set_overlay(0)
        e.set_tracking(0)


def test_overlay_off_behind_overlay_on_changes_nothing(net):
    e = net.engine
    frames = np.stack(vc.pipe_frames("480x640", 3))
    e.set_tracking(Engine.TRACK_ROWS)
    try:
        e.set_overlay(2)
        res_on, rows_on = submit_fetch(e, frames, 0)
        e.set_overlay(0)
        res_off, rows_off = submit_fetch(e, frames, 0)
        for (e1, k1, c1), (e2, k2, c2) in zip(res_on, res_off):
            assert np.array_equal(e1, e2) and np.array_equal(k1, k2) and np.array_equal(c1, c2)
        for r1, r2 in zip(rows_on, rows_off):
            assert all(np.array_equal(r1[k], r2[k]) for k in ("keypoints", "confidence", "bbox", "ids"))
        with pytest.raises(RuntimeError, match="ran without the overlay"):
            e.pipeline_overlay(0)
        e.set_overlay(1)
        e.set_tracking(0)
        with pytest.raises(RuntimeError, match="lwp_set_tracking mode >= 1"):
            e.pipeline_submit_u8(frames, 1, 368)
        e.set_tracking(Engine.TRACK_ROWS)
        e.pipeline_submit_u8(frames, 1, 368)
        with pytest.raises(RuntimeError, match="pipeline slot pending"):
            e.set_overlay(0)
        e.pipeline_fetch(1)
    finally:
        e.set_overlay(0)
        e.set_tracking(0)


def fields(poses):
    return (np.stack([p.keypoints for p in poses]) if poses else np.zeros((0, 18, 2), np.int32), [p.bbox for p in poses], [p.id for p in poses])


def test_run_demo_overlay_pipelined_equals_serial(net):
    base = vc.pipe_frames("480x640", 2)
    frames = base + [np.roll(f, 16, axis=1).copy() for f in base]
    runs = {}
    for key, kw in (("serial", dict()), ("pipelined", dict(pipelined=True))):
        pose_mod.Pose.last_id = -1
        given = [f.copy() for f in frames]
        runs[key] = list(demo.run_demo(net, given, 368, False, True, True, fused=True, device_tail=True, overlay=True, **kw))
        assert all(np.array_equal(g, f) for g, f in zip(given, frames))           # the provider's frames are unmodified
    pose_mod.Pose.last_id = -1
    assert len(runs["serial"]) == len(runs["pipelined"]) == 4
    changed = 0
    for t, ((si, sp), (pi, pp)) in enumerate(zip(runs["serial"], runs["pipelined"])):
        assert np.array_equal(si, pi), t
        fs, fp = fields(sp), fields(pp)
        assert np.array_equal(fs[0], fp[0]) and fs[1:] == fp[1:], t
        assert np.array_equal(pi, oc.render(frames[t], fp[0], np.array(fp[1]), DRAWN))
        changed += int((pi != frames[t]).any())
    assert changed >= 1
    with pytest.raises(RuntimeError, match="lwp_set_tracking|ran without|pose tail"):   # both settings are off again
        net.engine.pipeline_submit_u8(frames[0], 0, 368)
        net.engine.pipeline_fetch(0)
        net.engine.pipeline_overlay(0)


def test_run_cameras_overlay_equals_two_single_stream_runs(net):
    seqs = [vc.pipe_frames("480x640", 3, seed0=0), vc.pipe_frames("480x640", 3, seed0=5)]
    pose_mod.Pose.last_id = -1
    multi = list(demo.run_cameras(net, [[f.copy() for f in s] for s in seqs], 368, True, False, overlay=True))
    assert len(multi) == 3
    for l in range(2):
        pose_mod.Pose.last_id = -1
        single = list(demo.run_demo(net, [f.copy() for f in seqs[l]], 368, False, True, False, fused=True, device_tail=True,
                                    pipelined=True, overlay=True))
        for t in range(3):
            img, poses = multi[t][l]
            g, w = fields(poses), fields(single[t][1])
            assert np.array_equal(g[0], w[0]) and g[1:] == w[1:], (l, t)
            assert np.array_equal(img, single[t][0]), (l, t)
    pose_mod.Pose.last_id = -1
