"""Pose overlay, the parts that need no GPU (-m "not gpu"): the NumPy reference of tests/overlay_cases.py against the host
rasteriser ``Pose.draw``, the blend formula against round-to-nearest addWeighted, the new exports and their argument checks,
and run_demo's ``overlay`` keyword over a stub engine."""
import ctypes as C

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.modules.keypoints import BODY_PARTS_KPT_IDS

import overlay_cases as oc

COCO_CASES = [("edge_%dx%d" % s, s, oc.edge_poses(*s)) for s in oc.EDGE_SHAPES] + \
             [("long", (200, 320), oc.long_limb_poses()), ("crowd256", (16, 16), oc.crowd256())]


def test_the_reference_tables_are_the_packages():
    assert oc.COCO_LIMBS == [list(p) for p in BODY_PARTS_KPT_IDS]
    assert list(oc.COLOR) == list(pose_mod.Pose.color)


@pytest.mark.parametrize("name,shape,kps", COCO_CASES, ids=[c[0] for c in COCO_CASES])
def test_reference_painted_set_equals_pose_draw(name, shape, kps):
    h, w = shape
    frame = oc.noise_frames(1, h, w, seed=h * w)[0]
    frame[frame == pose_mod.Pose.color[0]] ^= 1         # no source byte equals a colour byte: painted <=> changed, per channel
    frame[frame == pose_mod.Pose.color[1]] ^= 1
    frame[frame == pose_mod.Pose.color[2]] ^= 1
    drawn = frame.copy()
    for kp in kps:
        pose_mod.Pose(kp.copy(), 1.0).draw(drawn)
    mask = oc.painted_mask(h, w, kps, oc.COCO_LIMBS[:-2])
    assert mask.any() and not mask.all()
    assert (drawn[mask] == pose_mod.Pose.color).all()               # painted pixels hold Pose.color
    assert np.array_equal(drawn[~mask], frame[~mask])               # untouched pixels stay untouched
    # and render is that set blended: out == src off the set, the formula on it
    out = oc.render(frame, kps, oc.bbox_of(kps), oc.COCO_LIMBS[:-2], boxes=False)
    assert np.array_equal(out[~mask], frame[~mask])
    assert np.array_equal(out[mask], ((6 * frame[mask].astype(int) + 4 * np.array(oc.COLOR) + 5) // 10).astype(np.uint8))


def test_far_outside_end_points_clip_to_the_step_range_pose_draw_walks():
    """2^20: the reference keeps only the steps near the frame; Pose.draw walks all two million of one limb (one limb, once)."""
    kps = oc.far_poses()
    one = kps.copy()
    one[0, [3, 4, 9, 10]] = -1                                      # keep (6,7): 2^20 -> inside, about a million steps
    frame = np.zeros((24, 40, 3), np.uint8)
    drawn = frame.copy()
    pose_mod.Pose(one[0].copy(), 1.0).draw(drawn)
    mask = oc.painted_mask(24, 40, one, oc.COCO_LIMBS[:-2])
    assert mask.sum() > 40 and np.array_equal(drawn[..., 1] == 224, mask)


def test_reference_boxes_equal_the_per_pixel_definition():
    """Outline pixels of render against the definition, pixel by pixel: rows y and y + h over x..x + w, columns x and x + w over
    y..y + h, clipped — on the crowd, whose boxes lie partly and wholly outside on every side."""
    kps = oc.crowd256()
    bb = oc.bbox_of(kps)
    frame = oc.noise_frames(1, 16, 16, seed=3)[0]
    frame[(frame == oc.BOX_COLOR).all(axis=-1)] = 7
    got = (oc.render(frame, kps[:0], bb, [], boxes=True) == oc.BOX_COLOR).all(axis=-1)
    want = np.zeros((16, 16), bool)
    for x, y, bw, bh in bb.tolist():
        for yy in range(16):
            for xx in range(16):
                if (yy in (y, y + bh) and x <= xx <= x + bw) or (xx in (x, x + bw) and y <= yy <= y + bh):
                    want[yy, xx] = True
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert any(x + bw < 0 and 0 <= y < 16 for x, y, bw, bh in bb.tolist())      # a box wholly to the left with a row inside


def test_blend_formula_is_round_to_nearest_add_weighted():
    o, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = (6 * o + 4 * c + 5) // 10
    assert np.array_equal(got, np.rint(0.6 * o.astype(np.float64) + 0.4 * c.astype(np.float64)).astype(int))
    f32 = np.float32(0.6) * o.astype(np.float32) + np.float32(0.4) * c.astype(np.float32)
    assert np.array_equal(got, np.rint(f32).astype(int))
    assert ((3 * o + 2 * c) % 5 * 2 != 5).all()                     # no ties: (3o + 2c) / 5 never ends in .5
    assert np.array_equal(((6 * o + 4 * o + 5) // 10), o)           # blending a pixel with itself maps it to itself


def test_exports_exist_and_the_version_moved():
    L = _lib.lib()
    for name in ("lwp_set_overlay", "lwp_get_overlay", "lwp_draw_poses"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.lwp_version() >= 102


def last_error():
    return _lib.lib().lwp_last_error(None).decode()


def test_set_overlay_argument_checks_without_a_handle():
    L = _lib.lib()
    for mode in (-1, 3):
        assert L.lwp_set_overlay(None, mode, None, None, 1, -1) == _lib.LWP_ERR_ARG and "overlay mode" in last_error()
    for nd in (-2, 20):
        assert L.lwp_set_overlay(None, 1, None, None, 1, nd) == _lib.LWP_ERR_ARG and "n_draw_limbs" in last_error()
    for nd in (-1, 0, 19):
        assert L.lwp_set_overlay(None, 2, None, None, 0, nd) == _lib.LWP_ERR_ARG and "handle is null" in last_error()


def test_draw_poses_argument_checks_without_a_handle():
    L = _lib.lib()
    ip = C.POINTER(C.c_int)
    img, out = np.zeros((2, 4, 5, 3), np.uint8), np.zeros((2, 4, 5, 3), np.uint8)
    n = np.array([1, 2], np.int32)
    kp, bb = np.zeros((2, 2, 18, 2), np.int32), np.zeros((2, 2, 4), np.int32)

    def call(imgs=img.ctypes.data, img_mem=0, N=2, H=4, W=5, n_poses=n, kps=kp, boxes=bb, cap=2, dst=out.ctypes.data, out_mem=0):
        as_ip = lambda a: a.ctypes.data_as(ip) if a is not None else None
        return L.lwp_draw_poses(None, imgs, img_mem, N, H, W, as_ip(n_poses), as_ip(kps), as_ip(boxes), cap, dst, out_mem)

    for kw, text in ((dict(imgs=None), "imgs / out is null"), (dict(dst=None), "imgs / out is null"),
                     (dict(dst=img.ctypes.data), "must not be imgs"), (dict(img_mem=2), "img_mem / out_mem"),
                     (dict(out_mem=-1), "img_mem / out_mem"), (dict(N=0), "N must be at least 1"), (dict(N=65536), "at most 65535"),
                     (dict(H=0), "empty frame"), (dict(W=0), "empty frame"), (dict(n_poses=None), "n_poses is null"),
                     (dict(cap=1), "frame 1 has 2 poses but pose_cap is 1"), (dict(cap=-1), "pose_cap"),
                     (dict(n_poses=np.array([0, -1], np.int32)), "frame 1 has -1 poses"),
                     (dict(kps=None), "keypoints / bbox is null"), (dict(boxes=None), "keypoints / bbox is null")):
        assert call(**kw) == _lib.LWP_ERR_ARG and text in last_error(), (kw, last_error())
    assert call() == _lib.LWP_ERR_ARG and "handle is null" in last_error()
    assert call(n_poses=np.zeros(2, np.int32), kps=None, boxes=None, cap=0) == _lib.LWP_ERR_ARG and "handle is null" in last_error()
    assert L.lwp_get_overlay(None, 2, out.ctypes.data, 0, 2, 4, 5) == _lib.LWP_ERR_ARG and "slot must be 0 or 1" in last_error()
    assert L.lwp_get_overlay(None, 0, None, 0, 2, 4, 5) == _lib.LWP_ERR_ARG and "dst is null" in last_error()


# ------------------------------------------------------------------------------------------ run_demo(overlay=...) over a stub
class StubEngine(object):
    """Records the calls of the loop; frame t (filled with t) yields one pose at (t, t + 1) and the annotated frame 255 - t."""
    TRACK_OFF, TRACK_ROWS, TRACK_LANES, TRACK_SEQUENCE = 0, 1, 2, 3
    OVERLAY_OFF, OVERLAY_DEVICE, OVERLAY_HOST = 0, 1, 2

    def __init__(self):
        self.log, self.slots, self.skeleton, self.overlay = [], {}, {"num_kpt_types": 18}, 0

    def set_tracking(self, mode, smooth=False, sigmas=None):
        self.log.append(("track", mode))

    def reset_tracking(self, lane, next_id):
        pass

    def set_overlay(self, mode, **kw):
        self.overlay = mode
        self.log.append(("overlay", mode, tuple(sorted(kw))))

    def pipeline_submit_u8(self, frames, slot, net_h, stride=8, upsample_ratio=4, demo=True):
        assert slot not in self.slots and self.overlay == self.OVERLAY_HOST
        f = np.asarray(frames)
        self.slots[slot] = f.reshape((-1,) + f.shape[-3:]).copy()
        self.log.append(("submit", slot))

    def pipeline_fetch(self, slot):
        self.fetched = (slot, self.slots.pop(slot))
        self.log.append(("fetch", slot))

    def _rows(self, t):
        kp = np.full((1, 18, 2), -1, np.int32)
        kp[0, 0] = (t, t + 1)
        return dict(keypoints=kp, confidence=np.array([1.0]), bbox=np.array([[t, t + 1, 1, 1]], np.int32), ids=np.array([100 + t], np.int32),
                    last_id=100 + t, near=0)

    def poses(self, slot=-1):
        assert slot == self.fetched[0]
        return [self._rows(int(f[0, 0, 0])) for f in self.fetched[1]]

    def pipeline_overlay(self, slot, device=False):
        assert slot == self.fetched[0]
        self.log.append(("overlay_of", slot))
        return 255 - self.fetched[1]


class Net(object):
    def __init__(self):
        self.engine = StubEngine()

    def eval(self):
        return self


def tagged(n, base=0):
    return [np.full((6, 8, 3), base + t, np.uint8) for t in range(n)]


def test_run_demo_overlay_needs_the_device_tail():
    for kw in (dict(), dict(fused=True), dict(device_tail=True)):
        with pytest.raises(ValueError, match="overlay=True"):
            demo.run_demo(Net(), [], 256, False, True, True, overlay=True, **kw)
    with pytest.raises(ValueError, match="unknown overlay option"):
        demo.run_demo(Net(), [], 256, False, True, True, fused=True, device_tail=True, overlay=dict(colour=(1, 2, 3)))


def test_run_demo_pipelined_overlay_yields_the_annotated_frames_in_order(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net, frames = Net(), tagged(5)
    out = list(demo.run_demo(net, frames, 256, False, True, False, fused=True, device_tail=True, pipelined=True,
                             overlay=dict(boxes=False)))
    assert len(out) == 5
    for t, (img, poses) in enumerate(out):
        assert img.shape == (6, 8, 3) and (img == 255 - t).all()     # the stub's annotated frame of frame t, not the provider's
        assert (frames[t] == t).all() and poses[0].keypoints[0].tolist() == [t, t + 1] and poses[0].id == 100 + t
    log = net.engine.log
    assert log[1] == ("overlay", 2, ("boxes",)) and log[-2:] == [("overlay", 0, ()), ("track", 0)]
    assert [e for e in log if e[0] == "overlay_of"] == [("overlay_of", t % 2) for t in range(5)]
    assert not net.engine.slots


def test_run_cameras_overlay_yields_one_annotated_frame_per_stream(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net = Net()
    provs = [tagged(3), tagged(3, base=50)]
    out = list(demo.run_cameras(net, provs, 256, True, False, overlay=True))
    assert len(out) == 3
    for t, step in enumerate(out):
        for l, (img, poses) in enumerate(step):
            assert (img == 255 - provs[l][t]).all() and poses[0].keypoints[0, 0] == provs[l][t][0, 0, 0]
    assert net.engine.log[-2:] == [("overlay", 0, ()), ("track", 0)]


def test_the_default_loops_never_touch_the_overlay(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net = Net()
    net.engine.overlay = StubEngine.OVERLAY_HOST                       # (only so that the stub's submit accepts the call)
    out = list(demo.run_demo(net, tagged(3), 256, False, True, False, fused=True, device_tail=True, pipelined=True))
    assert all(e[0] not in ("overlay", "overlay_of") for e in net.engine.log)
    assert all(img is f for (img, _), f in zip(out, tagged(0))) and len(out) == 3
