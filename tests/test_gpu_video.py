"""One-call video step on the GPU (-m gpu): the batched uint8 pre-processing kernel, lwp_pipeline_submit_u8 with its slot-scoped
un-map, run_demo(pipelined=True) and run_cameras.  Every comparison is exact unless it says otherwise.  Expected values come
from the oracle (oracle/preproc_ref.py, net_ref.py, post_ref.py, tail_ref.py through tests/video_cases.py); the serial exports
(preprocess_u8 -> set_unmap -> infer_poses -> poses) are a second, bit-exact cross-check.

As everywhere in this suite the network itself is held to the oracle network within NET_TOL (summation order differs) and
the integer / float64 stages are held to the oracle bit for bit on the maps they actually read: preproc_ref's tensor must equal
the device's, net_ref's maps bound the device's, post_ref on the device's maps must give the device's entries and key-points,
tail_ref on those must give the device's pose rows, boxes and ids."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo, synth
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine
from oracle import preproc_ref

import video_cases as vc

pytestmark = pytest.mark.gpu

NET_TOL = 1e-3

# the geometries of the single-frame test (tests/test_gpu_parity.py) plus one whose padded width is not a multiple of 4 (the
# kernel's one-pixel-per-thread form): no resize (368 x 656, 64 x 96), down-scaling (480, 721, 1080, 90), up-scaling (200, 333);
# none of the padded widths (656, 496, 552, 656, 456, 368, 96, 66) is a multiple of 256
GEOMETRIES = [(368, 656, 368, 8), (480, 640, 368, 8), (200, 300, 368, 8), (721, 1283, 368, 8), (1080, 1920, 256, 8),
              (333, 111, 368, 8), (64, 96, 64, 16), (90, 131, 45, 1)]


@functools.lru_cache(maxsize=None)
def base_frames(H, W):
    return synth.make_frames(3, H, W, seed0=H + W)


def distinct_frames(H, W, n):
    """n different frames from three seeded ones: frame i is base i % 3 rolled by 5 i pixels with i added (mod 256)."""
    base = base_frames(H, W)
    out = np.stack([np.roll(base[i % 3], 5 * i, axis=1) + np.uint8(i) for i in range(n)])
    assert len(set(f.tobytes() for f in out)) == n
    return np.ascontiguousarray(out)


@pytest.fixture(scope="module")
def net():
    n = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(n, {"state_dict": vc.state_dict()})
    return n.eval().cuda(0)


# ------------------------------------------------------------------------------------------ 1. batched pre-processing
@pytest.mark.parametrize("vec", ["0", "1"])
@pytest.mark.parametrize("N", [1, 3, 32])
@pytest.mark.parametrize("H,W,net_h,stride", GEOMETRIES)
def test_preprocess_u8_batch_is_bit_exact(monkeypatch, H, W, net_h, stride, N, vec):
    monkeypatch.setenv("LWP_PRE_BATCH_VEC", vec)
    eng = Engine(0)
    frames = distinct_frames(H, W, N)
    want = np.concatenate([preproc_ref.prepare_frame(f, net_h, stride)[0] for f in frames])
    _, scale, pad = preproc_ref.prepare_frame(frames[0], net_h, stride)
    x, scale2, pad2 = eng.preprocess_u8_batch(frames, net_h, stride)                         # host memory
    assert scale2 == scale and pad2 == pad and tuple(x.shape) == want.shape and x.dtype == torch.float32
    assert np.array_equal(x.cpu().numpy(), want)
    xd, _, _ = eng.preprocess_u8_batch(torch.from_numpy(frames).cuda(), net_h, stride)       # frames already in HBM
    assert np.array_equal(xd.cpu().numpy(), want)
    if N == 1:
        one, s1, p1 = eng.preprocess_u8(frames[0], net_h, stride)
        assert s1 == scale and p1 == pad and np.array_equal(one.cpu().numpy(), x.cpu().numpy())
        x3, _, _ = eng.preprocess_u8_batch(frames[0], net_h, stride)                         # (H, W, 3) is a batch of one
        assert np.array_equal(x3.cpu().numpy(), want)


@pytest.mark.parametrize("vec", ["0", "1"])
def test_preprocess_u8_batch_non_default_mean_scale_pad(monkeypatch, vec):
    monkeypatch.setenv("LWP_PRE_BATCH_VEC", vec)
    eng = Engine(0)
    frames = distinct_frames(240, 200, 3)
    kw = dict(pad_value=(3, 7.5, -2), img_mean=(104.5, 117, 123), img_scale=1 / 57.375)
    want = np.concatenate([preproc_ref.prepare_frame(f, 368, 8, **kw)[0] for f in frames])
    _, scale, pad = preproc_ref.prepare_frame(frames[0], 368, 8, **kw)
    for src in (frames, torch.from_numpy(frames).cuda()):
        x, scale2, pad2 = eng.preprocess_u8_batch(src, 368, 8, **kw)
        assert scale2 == scale and pad2 == pad and np.array_equal(x.cpu().numpy(), want)
    assert pad[1] > 0 and want[2, 1, 0, 0] == np.float32(7.5)
    one = eng.preprocess_u8(frames[1], 368, 8, **kw)[0]
    assert np.array_equal(one.cpu().numpy()[0], want[1])


def test_preprocess_u8_batch_host_frames_are_free_on_return_and_validation():
    eng = Engine(0)
    frames = distinct_frames(200, 300, 3)
    want = np.concatenate([preproc_ref.prepare_frame(f, 368, 8)[0] for f in frames])
    outs = []
    for _ in range(3):                                         # both pinned staging buffers, reused
        buf = frames.copy()
        x, _, _ = eng.preprocess_u8_batch(buf, 368, 8)
        buf[...] = 255 - buf
        outs.append(x)
    torch.cuda.synchronize()
    for x in outs:
        assert np.array_equal(x.cpu().numpy(), want)
    with pytest.raises(TypeError, match="uint8"):
        eng.preprocess_u8_batch(frames.astype(np.float32), 368, 8)
    with pytest.raises(TypeError, match="uint8"):
        eng.preprocess_u8_batch(frames[..., :2], 368, 8)
    with pytest.raises(TypeError, match="uint8"):
        eng.pipeline_submit_u8(frames.astype(np.int32), 0, 368)


# ------------------------------------------------------------------------------------------ helpers of the pipeline tests
def rows_of(r):
    return (r["keypoints"], r["bbox"], r["ids"], r["confidence"], r["last_id"])


def same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def serial_step(eng, frame, net_h=368, stride=8):
    """The parent's serial sequence for one frame: preprocess_u8 -> set_unmap -> infer_poses -> poses()."""
    x, scale, pad = eng.preprocess_u8(frame, net_h, stride, hand_over=False)
    eng.set_unmap(stride, scale, pad)
    ent, allk, _ = eng.infer_poses(x, 4, True)[0]
    return ent, allk, rows_of(eng.poses()[0]) if getattr(eng, "_tracking_mode", 0) else None


# ------------------------------------------------------------------------------------------ 2. one call against the oracle chain
@pytest.mark.parametrize("name", sorted(vc.PIPE_GEOMETRIES))
def test_pipeline_submit_u8_equals_the_oracle_chain_and_the_serial_sequence(net, name):
    eng = net.engine
    H, W, net_h, stride = vc.PIPE_GEOMETRIES[name]
    first = vc.pipe_frames(name, 2)
    # two steps of two lanes: every lane's second frame is its first one moved by 16 pixels (one cell of the stride-8 maps at
    # scale ~0.5), so ids are inherited and the filters move coordinates
    steps = [np.stack(first), np.stack([np.roll(f, 16, axis=1) for f in first])]
    try:
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        eng.set_unmap(16, 0.3, [7, 9, 0, 0])                   # the handle's un-map is deliberately another one: it must not be used
        got = []
        for k, batch in enumerate(steps):
            eng.pipeline_submit_u8(batch, k % 2, net_h, stride)
            res = eng.pipeline_fetch(k % 2)
            rows = eng.poses(k % 2)
            assert all(r["near"] == 0 for r in rows)
            got.append([(res[f][0], res[f][1], rows_of(rows[f])) for f in range(2)])
        tails = [vc.OracleTail(True, True), vc.OracleTail(True, True)]
        n_poses = inherited = 0
        for k, batch in enumerate(steps):
            maps = [vc.oracle_maps(batch[f], name) for f in range(2)]
            xd, _, _ = eng.preprocess_u8_batch(batch, net_h, stride)
            assert np.array_equal(xd.cpu().numpy(), np.concatenate([m[0] for m in maps]))   # preproc_ref, bit for bit
            outs = [o.cpu().numpy() for o in net(xd)]
            for f in range(2):
                x, heat_ref, paf_ref, scale, pad = maps[f]
                assert scale != 1.0 and pad[1] > 0
                assert np.abs(outs[-2][f] - heat_ref).max() <= NET_TOL and np.abs(outs[-1][f] - paf_ref).max() <= NET_TOL   # net_ref
                ent, allk = vc.oracle_post(outs[-2][f], outs[-1][f])                     # post_ref on the maps the grouping read
                g_ent, g_allk, g_rows = got[k][f]
                assert np.array_equal(g_ent, ent) and np.array_equal(g_allk, allk)
                want = tails[f].step(ent, allk, scale, pad, stride, 4)                   # tail_ref
                assert same_rows(g_rows, want), (k, f)
                n_poses += len(ent)
                if k == 1:
                    inherited += len(set(g_rows[2].tolist()) & set(got[0][f][2][2].tolist()))
        assert n_poses >= 8 and inherited > 0
        # the parent's serial sequence on the same batch, bit for bit: preprocess_u8 per frame -> set_unmap -> infer_poses -> poses()
        # (the same batch size: the fp32 network picks its kernels by problem size, so its maps — and with them the float scores in
        # the entries — depend on the batch size at the 1e-6 level, see lwp_forward in include/lwpose.h)
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        for k, batch in enumerate(steps):
            pre = [eng.preprocess_u8(f, net_h, stride) for f in batch]
            eng.set_unmap(stride, pre[0][1], pre[0][2])
            res = eng.infer_poses(torch.cat([p[0] for p in pre]), 4, True)
            rows = eng.poses()
            for f in range(2):
                assert np.array_equal(res[f][0], got[k][f][0]) and np.array_equal(res[f][1], got[k][f][1]), (k, f)
                assert same_rows(rows_of(rows[f]), got[k][f][2]), (k, f)
    finally:
        eng.synchronize()
        eng.set_tracking(Engine.TRACK_OFF)
        eng.set_unmap(8, 1.0, [0, 0, 0, 0])


# ------------------------------------------------------------------------------------------ 3. tail off
def test_tail_off_equals_preprocess_plus_pipeline_submit(net):
    eng = net.engine
    frames = np.stack(vc.pipe_frames("720x1280", 3))
    eng.pipeline_submit_u8(frames, 1, 368, 8)
    got = eng.pipeline_fetch(1)
    with pytest.raises(RuntimeError, match="pose tail was off"):
        eng.poses(1)
    x = torch.cat([eng.preprocess_u8(f, 368, 8)[0] for f in frames])
    eng.pipeline_submit(x, 0)
    want = eng.pipeline_fetch(0)
    assert sum(len(w[0]) for w in want) >= 6
    for g, w in zip(got, want):
        assert all(np.array_equal(a, b) for a, b in zip(g, w))
    n = np.zeros(3, np.int32)
    ip = C.POINTER(C.c_int)
    bufs = [np.zeros(3 * 256 * 36, np.int32) for _ in range(3)]
    conf = np.zeros(3 * 256, np.float64)
    rc = _lib.lib().lwp_get_poses(eng.h.ptr, 1, n.ctypes.data_as(ip), bufs[0].ctypes.data_as(ip), conf.ctypes.data_as(C.POINTER(C.c_double)),
                                  bufs[1].ctypes.data_as(ip), bufs[2].ctypes.data_as(ip), None, 256)
    assert rc == _lib.LWP_ERR_STATE


# ------------------------------------------------------------------------------------------ 4. slot-scoped un-map
def test_submit_unmap_is_scoped_to_the_slot(net):
    eng = net.engine
    frame = vc.pipe_frames("480x640", 1)[0]
    _, _, _, _, pad, scale = Engine.preprocess_dims(480, 640, 368, 8)
    other = (16, 0.37, [5, 11, 0, 0])
    try:
        eng.set_tracking(Engine.TRACK_ROWS)
        eng.set_unmap(*other)
        eng.pipeline_submit_u8(frame, 0, 368, 8)
        ent, allk, _ = eng.pipeline_fetch(0)[0]
        sub = rows_of(eng.poses(0)[0])
        x, _, _ = eng.preprocess_u8(frame, 368, 8)
        ent2, allk2, _ = eng.infer_poses(x, 4, True)[0]          # no set_unmap in between: the handle's values hold
        ser = rows_of(eng.poses()[0])
        assert np.array_equal(ent, ent2) and np.array_equal(allk, allk2) and len(ent) >= 2
        assert same_rows(sub, vc.OracleTail(False, False).step(ent, allk, scale, pad, 8, 4))
        assert same_rows(ser, vc.OracleTail(False, False).step(ent, allk, other[1], other[2], other[0], 4))
        assert not np.array_equal(sub[0], ser[0])
    finally:
        eng.set_tracking(Engine.TRACK_OFF)
        eng.set_unmap(8, 1.0, [0, 0, 0, 0])


# ------------------------------------------------------------------------------------------ 5. two slots in flight, geometry changes
def test_two_slots_in_flight_with_alternating_frame_sizes(net):
    eng = net.engine
    a, b = vc.pipe_frames("720x1280", 4, seed0=3), vc.pipe_frames("480x640", 4, seed0=7)
    frames = [a[0], b[0], a[1], b[1], np.roll(a[1], 16, axis=1), np.roll(b[1], 16, axis=1), a[2], b[2]]
    try:
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        serial = [serial_step(eng, f) for f in frames]
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        got = []

        def fetch(k):
            ent, allk, _ = eng.pipeline_fetch(k % 2)[0]
            got.append((ent, allk, rows_of(eng.poses(k % 2)[0])))
        eng.pipeline_submit_u8(frames[0], 0, 368, 8)
        for k in range(1, len(frames)):
            buf = frames[k].copy()
            eng.pipeline_submit_u8(buf, k % 2, 368, 8)                                  # submit(k) before fetch(k - 1)
            buf[...] = 0                                                                # a host frame is free on return
            fetch(k - 1)
        fetch(len(frames) - 1)
        assert len(got) == len(frames) >= 6
        for k, (s, g) in enumerate(zip(serial, got)):
            assert np.array_equal(s[0], g[0]) and np.array_equal(s[1], g[1]) and same_rows(s[2], g[2]), k
            assert len(g[0]) >= 2, k
    finally:
        eng.synchronize()
        eng.set_tracking(Engine.TRACK_OFF)


def test_chunked_batch_equals_separate_submits_of_the_chunk_size(monkeypatch, net):
    """A batch walked in passes of 2 frames gives the bits of two submits of 2 frames (the network's kernels are chosen by the
    frames per pass, so the comparison is at the same pass size, as for lwp_forward's 140 = 2 x 70 frames)."""
    frames = np.stack(vc.pipe_frames("480x640", 4))
    eng = net.engine
    want, want_rows = [], []
    try:
        eng.set_tracking(Engine.TRACK_ROWS)
        for half in (frames[:2], frames[2:]):
            eng.pipeline_submit_u8(half, 0, 368, 8)
            want += [(r[0], r[1]) for r in eng.pipeline_fetch(0)]
            want_rows += [rows_of(r) for r in eng.poses(0)]
    finally:
        eng.set_tracking(Engine.TRACK_OFF)
    monkeypatch.setenv("LWP_MAX_FRAMES_PER_PASS", "3")
    n2 = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(n2, {"state_dict": vc.state_dict()})
    e2 = n2.eval().cuda(0).engine
    assert e2.frames_per_pass(4, 368, 496) == 2
    e2.set_tracking(Engine.TRACK_ROWS)
    e2.pipeline_submit_u8(torch.from_numpy(frames).cuda(), 1, 368, 8)                    # device frames
    got = e2.pipeline_fetch(1)
    for f in range(4):
        assert np.array_equal(got[f][0], want[f][0]) and np.array_equal(got[f][1], want[f][1])
        assert same_rows(rows_of(e2.poses(1)[f]), want_rows[f])
    assert sum(len(w[0]) for w in want) >= 8


# ------------------------------------------------------------------------------------------ 6. tracking through run_demo / run_cameras
def moving_frames(seed0, n=6):
    base = [np.ascontiguousarray(f) for f in synth.make_frames(n // 2, 720, 1280, seed0=seed0)]
    return base + [np.roll(f, 16, axis=1).copy() for f in base]


def collect(gen):
    return [(np.stack([p.keypoints for p in poses]), [p.bbox for p in poses], [p.id for p in poses], [p.confidence for p in poses])
            for _, poses in gen]


@pytest.mark.parametrize("smooth", [False, True])
def test_run_demo_pipelined_equals_serial_device_tail_and_python_tail(net, smooth):
    frames = moving_frames(0, 8)
    runs, last = {}, {}
    for key, kw in (("python", dict(fused=True)), ("serial", dict(fused=True, device_tail=True)),
                    ("pipelined", dict(fused=True, device_tail=True, pipelined=True))):
        pose_mod.Pose.last_id = -1
        runs[key] = collect(demo.run_demo(net, [f.copy() for f in frames], 368, False, True, smooth, **kw))
        last[key] = pose_mod.Pose.last_id
    pose_mod.Pose.last_id = -1
    assert last["pipelined"] == last["serial"] == last["python"] >= 0
    assert len(runs["pipelined"]) == len(frames)
    for t in range(len(frames)):
        for other in ("serial", "python"):
            w, g = runs[other][t], runs["pipelined"][t]
            assert np.array_equal(w[0], g[0]) and w[1] == g[1] and w[2] == g[2] and w[3] == g[3], (other, t)
    ids = [set(r[2]) for r in runs["pipelined"]]
    assert len(runs["pipelined"][0][2]) >= 2 and any(ids[t] & ids[t - 1] for t in range(1, len(frames)))
    # the tracking setting is off again and no slot is pending
    net.engine.pipeline_submit_u8(frames[0], 0, 368)
    net.engine.pipeline_fetch(0)
    with pytest.raises(RuntimeError, match="pose tail was off"):
        net.engine.poses(0)


def test_run_demo_pipelined_closed_early_leaves_the_engine_idle(net):
    frames = moving_frames(0, 4)
    pose_mod.Pose.last_id = -1
    gen = demo.run_demo(net, frames, 368, False, True, True, fused=True, device_tail=True, pipelined=True)
    next(gen)
    gen.close()
    pose_mod.Pose.last_id = -1
    eng = net.engine
    eng.set_tracking(Engine.TRACK_ROWS)                           # would be refused with a slot pending
    eng.set_tracking(Engine.TRACK_OFF)
    for slot in (0, 1):
        with pytest.raises(RuntimeError, match="nothing submitted"):
            eng.pipeline_fetch(slot)


def pose_fields(poses):
    return (np.stack([p.keypoints for p in poses]), [p.bbox for p in poses], [p.id for p in poses], [p.confidence for p in poses])


def camera_sequences():
    seqs = [moving_frames(10 * (l + 1), 6) for l in range(4)]
    seqs[2] = seqs[2][:5]                                         # the shortest provider ends the run
    return seqs


def test_run_cameras_equals_four_single_lane_runs(monkeypatch):
    """Lane f of run_cameras equals run_demo's device-tail run over provider f alone in EVERY field, the float confidence
    included.  The fp32 network picks its kernels by the frames of a pass, so the engine here walks a batch one frame per pass
    (LWP_MAX_FRAMES_PER_PASS=1, the switch the chunking test uses): its batch-4 step runs the kernels of the single-lane run,
    and upload, batched pre-processing, lane ownership, tail and result rows are those of any run_cameras step."""
    monkeypatch.setenv("LWP_MAX_FRAMES_PER_PASS", "1")
    n1 = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(n1, {"state_dict": vc.state_dict()})
    n1 = n1.eval().cuda(0)
    assert n1.engine.frames_per_pass(4, 368, 656) == 1
    seqs = camera_sequences()
    pose_mod.Pose.last_id = -1
    multi = list(demo.run_cameras(n1, [[f.copy() for f in s] for s in seqs], 368, True, True))
    assert pose_mod.Pose.last_id == -1 and len(multi) == 5 and all(len(step) == 4 for step in multi)
    total = 0
    for l in range(4):
        pose_mod.Pose.last_id = -1
        single = collect(demo.run_demo(n1, [f.copy() for f in seqs[l][:5]], 368, False, True, True, fused=True, device_tail=True))
        for t in range(5):
            img, poses = multi[t][l]
            assert np.array_equal(img, seqs[l][t])
            g, w = pose_fields(poses), single[t]
            assert np.array_equal(w[0], g[0]) and w[1] == g[1] and w[2] == g[2] and w[3] == g[3], (l, t)
            total += len(poses)
    pose_mod.Pose.last_id = -1
    assert total >= 40


def test_run_cameras_at_batch_4_equals_the_serial_four_lane_loop(net):
    """The default engine, whose batch-4 step runs the batch-4 kernels: every field of every lane, the confidence included,
    equals the serial exports driven as four lanes at the same batch size (preprocess_u8 x 4 -> set_unmap -> infer_poses ->
    poses()) bit for bit, and each lane's key-points, boxes and ids are those of a single-lane run."""
    eng = net.engine
    seqs = camera_sequences()
    pose_mod.Pose.last_id = 6                                     # every lane starts at Pose.last_id + 1
    multi = list(demo.run_cameras(net, [[f.copy() for f in s] for s in seqs], 368, True, True))
    assert pose_mod.Pose.last_id == 6 and len(multi) == 5
    total = 0
    try:
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        eng.reset_tracking(-1, 7)
        for t in range(5):
            pre = [eng.preprocess_u8(seqs[l][t], 368, 8) for l in range(4)]
            eng.set_unmap(8, pre[0][1], pre[0][2])
            eng.infer_poses(torch.cat([p[0] for p in pre]), 4, True)
            rows = eng.poses()
            for l in range(4):
                g, r = pose_fields(multi[t][l][1]), rows[l]
                assert np.array_equal(g[0], r["keypoints"]) and g[1] == [tuple(b) for b in r["bbox"].tolist()], (l, t)
                assert g[2] == r["ids"].tolist() and g[3] == r["confidence"].tolist() and min(g[2]) >= 7, (l, t)
                total += len(g[2])
    finally:
        pose_mod.Pose.last_id = -1
        eng.set_tracking(Engine.TRACK_OFF)
        eng.set_unmap(8, 1.0, [0, 0, 0, 0])
    for l in range(4):
        pose_mod.Pose.last_id = 6
        single = collect(demo.run_demo(net, [f.copy() for f in seqs[l][:5]], 368, False, True, True, fused=True, device_tail=True))
        pose_mod.Pose.last_id = -1
        for t in range(5):
            g, w = pose_fields(multi[t][l][1]), single[t]
            assert np.array_equal(w[0], g[0]) and w[1] == g[1] and w[2] == g[2], (l, t)      # the integer fields; the confidence: the test above
    assert total >= 40


# ------------------------------------------------------------------------------------------ 7. state
def test_state_rules_of_the_one_call_submit(net):
    eng = net.engine
    frame = vc.pipe_frames("480x640", 1)[0]
    x, _, _ = eng.preprocess_u8(frame, 368, 8)
    try:
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        eng.pipeline_submit_u8(frame, 0, 368)
        with pytest.raises(RuntimeError, match="pending"):
            eng.pipeline_submit_u8(frame, 0, 368)                  # the slot is pending
        with pytest.raises(RuntimeError, match="pipeline slot is pending"):
            eng.infer_poses(x, 4, True)                            # serial exports: the lanes belong to the slot's stream
        with pytest.raises(RuntimeError, match="pending"):
            eng.set_tracking(Engine.TRACK_OFF)
        with pytest.raises(RuntimeError, match="pending"):
            eng.poses(0)
        eng.pipeline_submit_u8(frame, 1, 368)                      # the other slot is free
        eng.pipeline_fetch(0)
        eng.pipeline_fetch(1)
        a, b = eng.poses(0)[0], eng.poses(1)[0]
        assert len(a["ids"]) >= 2 and sorted(a["ids"].tolist()) == sorted(b["ids"].tolist())      # the same frame twice: every id carried over
        with pytest.raises(ValueError, match="slot"):
            eng.pipeline_submit_u8(frame, 2, 368)
        with pytest.raises(ValueError, match="upsample ratio"):
            eng.pipeline_submit_u8(frame, 0, 368, upsample_ratio=2)
        with pytest.raises(ValueError, match="frame too small"):
            eng.pipeline_submit_u8(np.zeros((4, 4, 3), np.uint8), 0, 4, stride=1)
        eng.infer_poses(x, 4, True)                                # nothing pending: the serial path works again
    finally:
        eng.synchronize()
        eng.set_tracking(Engine.TRACK_OFF)
    big = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(big, {"state_dict": vc.state_dict()})
    be = big.eval().cuda(0).engine
    be.set_capacity(max_entries=300)
    be.set_tracking(Engine.TRACK_ROWS)
    with pytest.raises(ValueError, match="256 poses"):
        be.pipeline_submit_u8(frame, 0, 368)
    be.set_tracking(Engine.TRACK_OFF)
    fresh = Engine(0)
    with pytest.raises(RuntimeError, match="weights not loaded"):
        fresh.pipeline_submit_u8(frame, 0, 368)
