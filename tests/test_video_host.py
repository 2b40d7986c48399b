"""CPU: the one-call video step — the two batched uint8 exports' argument checks (no GPU, no handle), the submit / fetch order
of ``run_demo(pipelined=True)`` and ``run_cameras`` against a recording engine, and — with the oracle alone — that the frames
tests/test_gpu_video.py runs yield poses under a non-trivial scale and pad."""
import ctypes as C

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo, synth
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.runtime import Engine

import video_cases as vc

NEW_EXPORTS = ["lwp_preprocess_u8_batch", "lwp_pipeline_submit_u8"]


def _err():
    return _lib.lib().lwp_last_error(None).decode()


def _d3(*v):
    return (C.c_double * 3)(*v)


def test_new_exports_exist_and_are_declared():
    L = _lib.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name


def _batch(imgs=True, N=1, H=720, W=1280, net_h=368, stride=8, pv=True, mean=True, out=True, mem=0):
    buf = np.zeros(16, np.uint8)
    dst = np.zeros(16, np.float32)
    return _lib.lib().lwp_preprocess_u8_batch(None, buf.ctypes.data if imgs else None, mem, N, H, W, net_h, stride,
                                              _d3(0, 0, 0) if pv else None, _d3(128, 128, 128) if mean else None, 1 / 256,
                                              dst.ctypes.data if out else None)


def _submit(imgs=True, N=1, H=720, W=1280, net_h=368, stride=8, pv=True, mean=True, ratio=4, slot=0, mem=0):
    buf = np.zeros(16, np.uint8)
    return _lib.lib().lwp_pipeline_submit_u8(None, buf.ctypes.data if imgs else None, mem, N, H, W, net_h, stride,
                                             _d3(0, 0, 0) if pv else None, _d3(128, 128, 128) if mean else None, 1 / 256, ratio, 1, slot)


@pytest.mark.parametrize("call", [_batch, _submit])
def test_argument_checks_run_without_a_handle(call):
    E = _lib.LWP_ERR_ARG
    assert call(imgs=False) == E and "imgs is null" in _err()
    assert call(pv=False) == E and "pad_value" in _err()
    assert call(mean=False) == E and "img_mean" in _err()
    assert call(mem=2) == E and "img_mem" in _err()
    for n in (0, -3):
        assert call(N=n) == E and "N must be at least 1" in _err()
    assert call(N=65536) == E and "65535" in _err()
    assert call(H=0) == E and "bad frame" in _err()
    assert call(W=-1) == E and "bad frame" in _err()
    assert call(stride=0) == E and "bad frame" in _err()
    assert call(H=4000, W=2, net_h=8) == E and "bad frame" in _err()            # the scaled frame is empty
    # the padded frame is what the network sees: it needs 8 x 8
    assert call(H=4, W=4, net_h=4, stride=1) == E and "frame too small" in _err() and "4 x 4" in _err()
    assert call(H=100, W=100, net_h=7, stride=1) == E and "frame too small" in _err()
    # everything valid: the handle is what is missing
    assert call() == E and "handle is null" in _err()
    assert call(H=8, W=8, net_h=8, stride=8) == E and "handle is null" in _err()


def test_output_pointer_slot_and_ratio_checks():
    E = _lib.LWP_ERR_ARG
    assert _batch(out=False) == E and "out_device is null" in _err()
    for slot in (-1, 2):
        assert _submit(slot=slot) == E and "slot must be 0 or 1" in _err()
    assert _submit(ratio=3) == E and "upsample ratio" in _err()


def test_padding_is_never_negative():
    """Both exports refuse a negative pad (LWP_ERR_ARG "negative padding").  lwp_preprocess_dims cannot produce one — the scaled
    height is the network height, the padded sizes are rounded UP to the stride — so the refusal is a guard, and this is the
    property it rests on, over the geometries a caller can name."""
    rng = np.random.RandomState(3)
    for _ in range(2000):
        H, W = int(rng.randint(1, 2200)), int(rng.randint(1, 4000))
        net_h, stride = int(rng.randint(1, 1100)), int(rng.choice([1, 2, 3, 4, 8, 16, 32, 64]))
        try:
            dh, dw, oh, ow, pad, scale = Engine.preprocess_dims(H, W, net_h, stride)
        except ValueError:
            continue                                   # an empty scaled frame
        assert min(pad) >= 0 and oh == dh + pad[0] + pad[2] and ow == dw + pad[1] + pad[3] and oh % stride == 0 and ow % stride == 0


# ------------------------------------------------------------------------------------------ run_demo(pipelined=True) ordering
class Recorder(object):
    """Records the calls the pipelined loops make; the poses of frame t carry t in their first key-point and confidence."""
    TRACK_OFF, TRACK_ROWS, TRACK_LANES, TRACK_SEQUENCE = 0, 1, 2, 3
    skeleton = {"num_kpt_types": 18}

    def __init__(self):
        self.log, self.slots, self.mode = [], {}, 0

    def set_tracking(self, mode, smooth=False, sigmas=None):
        if self.slots:
            raise RuntimeError("pipeline slot pending")
        self.mode = mode
        self.log.append(("track", mode))

    def reset_tracking(self, lane, next_id):
        self.log.append(("reset", lane, next_id))

    def pipeline_submit_u8(self, frames, slot, height, stride=8, upsample_ratio=4, demo=True, **kw):
        assert self.mode != 0, "submitted with the tail off"
        assert slot not in self.slots, "slot reused before it was fetched"
        a = np.asarray(frames)
        tags = [int(a[0, 0, 0])] if a.ndim == 3 else [int(f[0, 0, 0]) for f in a]
        self.slots[slot] = tags
        self.log.append(("submit", slot, tuple(tags)))

    def pipeline_fetch(self, slot):
        self.fetched = (slot, self.slots.pop(slot))
        self.log.append(("fetch", slot))

    def poses(self, slot):
        assert self.fetched[0] == slot
        out = []
        for tag in self.fetched[1]:
            kp = np.full((1, 18, 2), -1, np.int32)
            kp[0, 0] = (tag, tag + 1)
            out.append(dict(keypoints=kp, confidence=np.array([float(tag)]), bbox=np.array([[tag, tag + 1, 1, 1]], np.int32),
                            ids=np.array([100 + tag], np.int32), last_id=100 + tag, near=0))
        return out

    def __getattr__(self, name):
        raise AssertionError("unexpected engine call: %s" % name)


class Net(object):
    def __init__(self):
        self.engine = Recorder()

    def eval(self):
        return self


def tagged_frames(n, h=6, w=8, base=0):
    return [np.full((h, w, 3), base + t, np.uint8) for t in range(n)]


def test_run_demo_pipelined_needs_device_tail():
    with pytest.raises(ValueError, match="device_tail=True"):
        demo.run_demo(Net(), [], 256, False, True, True, fused=True, pipelined=True)
    with pytest.raises(ValueError, match="device_tail=True"):
        demo.run_demo(Net(), [], 256, False, True, True, pipelined=True)


def test_run_demo_pipelined_submit_fetch_order_and_pairing(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", 6)
    net = Net()
    frames = tagged_frames(5)
    out = list(demo.run_demo(net, frames, 256, False, True, True, fused=True, device_tail=True, pipelined=True))
    log = net.engine.log
    assert log[0] == ("track", Recorder.TRACK_LANES) and log[1] == ("reset", 0, 7) and log[-1] == ("track", Recorder.TRACK_OFF)
    assert log[2:-1] == [("submit", 0, (0,)), ("submit", 1, (1,)), ("fetch", 0), ("submit", 0, (2,)), ("fetch", 1), ("submit", 1, (3,)),
                         ("fetch", 0), ("submit", 0, (4,)), ("fetch", 1), ("fetch", 0)]
    assert len(out) == 5 and not net.engine.slots
    for t, (img, poses) in enumerate(out):
        assert img is frames[t]                                   # the frame that belongs to the poses
        assert len(poses) == 1 and poses[0].keypoints[0].tolist() == [t, t + 1] and poses[0].id == 100 + t
    assert pose_mod.Pose.last_id == 104


def test_run_demo_pipelined_one_frame_and_no_frames(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net = Net()
    assert list(demo.run_demo(net, [], 256, False, False, False, fused=True, device_tail=True, pipelined=True)) == []
    assert net.engine.log == [("track", Recorder.TRACK_ROWS), ("track", Recorder.TRACK_OFF)]
    net = Net()
    out = list(demo.run_demo(net, tagged_frames(1), 256, False, False, False, fused=True, device_tail=True, pipelined=True))
    assert len(out) == 1 and out[0][1][0].id is None              # no tracking: no ids
    assert net.engine.log[1:-1] == [("submit", 0, (0,)), ("fetch", 0)]


def test_run_demo_pipelined_early_close_fetches_the_pending_slot(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net = Net()
    gen = demo.run_demo(net, tagged_frames(6), 256, False, True, False, fused=True, device_tail=True, pipelined=True)
    img, poses = next(gen)
    assert poses[0].keypoints[0, 0] == 0 and net.engine.slots == {1: [1]}         # frame 1 is in flight while frame 0 is out
    gen.close()
    assert not net.engine.slots
    assert net.engine.log[-2:] == [("fetch", 1), ("track", Recorder.TRACK_OFF)]
    assert net.engine.mode == Recorder.TRACK_OFF


def test_run_demo_pipelined_draws_on_the_frame_of_the_poses(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    drawn = []
    monkeypatch.setattr(pose_mod.Pose, "draw", lambda self, img: drawn.append((int(img[0, 0, 0]), int(self.keypoints[0, 0]))))
    list(demo.run_demo(Net(), tagged_frames(4), 256, False, True, False, fused=True, device_tail=True, pipelined=True, draw=True))
    assert drawn == [(t, t) for t in range(4)]


def test_default_run_demo_is_untouched_by_the_new_keyword():
    import inspect
    sig = inspect.signature(demo.run_demo)
    assert sig.parameters["pipelined"].default is False
    assert list(sig.parameters)[:10] == ["net", "image_provider", "height_size", "cpu", "track", "smooth", "fused", "draw", "device_tail", "sigmas"]


def test_run_cameras_batches_lanes_and_stops_with_the_first_provider(monkeypatch):
    monkeypatch.setattr(pose_mod.Pose, "last_id", 9)
    net = Net()
    provs = [tagged_frames(4, base=0), tagged_frames(3, base=50), tagged_frames(5, base=100)]
    out = list(demo.run_cameras(net, provs, 256, True, True))
    log = net.engine.log
    assert log[0] == ("track", Recorder.TRACK_LANES) and log[1] == ("reset", -1, 10) and log[-1] == ("track", Recorder.TRACK_OFF)
    assert log[2:-1] == [("submit", 0, (0, 50, 100)), ("submit", 1, (1, 51, 101)), ("fetch", 0), ("submit", 0, (2, 52, 102)),
                         ("fetch", 1), ("fetch", 0)]
    assert len(out) == 3 and all(len(step) == 3 for step in out)
    for t, step in enumerate(out):
        for l, (img, poses) in enumerate(step):
            assert img is provs[l][t] and poses[0].keypoints[0, 0] == provs[l][t][0, 0, 0]
    assert pose_mod.Pose.last_id == 9                             # ids are per lane: the shared counter is left alone
    with pytest.raises(ValueError, match="same-sized"):
        list(demo.run_cameras(Net(), [tagged_frames(2), tagged_frames(2, h=7)], 256, True, False))


def test_run_cameras_checks_its_arguments_at_the_call():
    with pytest.raises(ValueError, match="at least one provider"):
        demo.run_cameras(Net(), [], 256, True, True)               # no next(): the call itself raises, like run_demo's
    net = Net()
    net.engine.skeleton = {"num_kpt_types": 5}
    with pytest.raises(ValueError, match="give sigmas"):
        demo.run_cameras(net, [tagged_frames(2)], 256, True, True)
    assert net.engine.log == []


class FailingFetch(Recorder):
    def pipeline_fetch(self, slot):
        self.slots.pop(slot)
        self.log.append(("fetch", slot))
        raise RuntimeError("hip error in slot %d" % slot)


@pytest.mark.parametrize("cameras", [False, True])
def test_an_error_of_the_closing_fetch_is_raised_after_tracking_is_off(monkeypatch, cameras):
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    net = Net()
    if cameras:
        gen = demo.run_cameras(net, [tagged_frames(4), tagged_frames(4, base=50)], 256, True, False)
    else:
        gen = demo.run_demo(net, tagged_frames(4), 256, False, True, False, fused=True, device_tail=True, pipelined=True)
    next(gen)
    net.engine.__class__ = FailingFetch
    with pytest.raises(RuntimeError, match="hip error in slot 1"):
        gen.close()
    assert net.engine.log[-2:] == [("fetch", 1), ("track", Recorder.TRACK_OFF)] and not net.engine.slots


# ------------------------------------------------------------------------------------------ the GPU tests' frames, by the oracle alone
def test_gpu_frames_have_a_non_trivial_geometry():
    for name, (H, W, net_h, stride) in vc.PIPE_GEOMETRIES.items():
        dh, dw, oh, ow, pad, scale = Engine.preprocess_dims(H, W, net_h, stride)
        assert scale != 1.0 and (pad[0] > 0 or pad[1] > 0), name
        # the un-map must matter: a key-point at the map centre lands elsewhere with the handle's defaults (8, 1.0, 0, 0)
        x = ow // 2
        assert int((x * 8 / 4 - pad[1]) / scale) != int(x * 8 / 4), name


@pytest.mark.parametrize("name", sorted(vc.PIPE_GEOMETRIES))
def test_gpu_frames_yield_poses_in_the_oracle_chain(name):
    """preproc_ref -> net_ref -> post_ref on the frames of the one-call pipeline test: every geometry has frames with poses."""
    frames = vc.pipe_frames(name, 2)
    found = [len(vc.oracle_chain(f, name)[0]) for f in frames]
    assert min(found) >= 2, found
