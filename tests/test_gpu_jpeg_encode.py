"""GPU: the JPEG encoder (csrc/jpeg_encode_kernels.hip behind lwp_jpeg_encode_batch) against the files Pillow wrote
of the fixtures' pixels, byte for byte: every fixture in one call per setting, alone and again, from host arrays and from cuda
tensors; the first stage's coefficients against the NumPy restatement; a capacity too small in the middle of a batch; a caller's
side stream; what a closed engine gives back; the way back through the decoder; Motion-JPEG files written and read on the card;
run_demo fed by VideoReader; the annotated frame kept on the device; the command line as a fresh child process."""
import ctypes
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.datasets import coco
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import jpeg_cases as jc
import jpeg_encode_cases as jen
import video_cases as vc

from conftest import ROOT

pytestmark = pytest.mark.gpu
FIX = jen.fixtures()
NAMES = sorted(FIX)
# the stages' granularities (csrc/lwp_internal.h): 32 blocks a workgroup of the first stage, kJpegEncGroup = 256 blocks a
# workgroup of the length and write passes and a tile of the offset scan, kJpegEncGroup * kJpegEncChunk = 8192 un-stuffed bytes a
# tile of the stuffing passes; the long fixture spans more than one of each on its own (test_jpeg_encode_host.py checks it)
ENC_GROUP, ENC_CHUNK = 256, 32


def settings():
    """{(quality, sampling, restart): [names]}: a call has one setting, so the fixtures go in one call per setting."""
    out = {}
    for n in NAMES:
        out.setdefault((FIX[n]["quality"], FIX[n]["sampling"], FIX[n]["restart"]), []).append(n)
    return out


@pytest.fixture(scope="module")
def eng():
    return Engine(0, nref=1, num_channels=32)          # the encoder needs no weights


@pytest.fixture(scope="module")
def batches(eng):
    """{name: bytes} of every fixture, encoded from HOST arrays with all fixtures of a setting in ONE call: sizes from 1x1 to
    100x75 mixed, so image boundaries fall inside the workgroups of every stage."""
    out = {}
    for (q, s, r), names in settings().items():
        for n, data in zip(names, eng.encode_jpeg_batch([FIX[n]["bgr"] for n in names], q, s, r)):
            out[n] = data
    return out


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def test_every_fixture_batched_by_setting_equals_pillows_file_in_every_byte(batches):
    assert len(batches) == len(NAMES) > 50 and max(len(v) for v in settings().values()) >= 3
    for n in NAMES:
        got, want = batches[n], FIX[n]["jpeg"]
        assert isinstance(got, bytes)
        assert got == want, "%s: %d bytes against %d, first difference at %d" % (n, len(got), len(want), first_difference(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_each_fixture_alone_from_a_cuda_tensor_equals_pillows_file(eng, name):
    f = FIX[name]
    got = eng.encode_jpeg_batch([torch.from_numpy(f["bgr"]).cuda()], f["quality"], f["sampling"], f["restart"])
    assert len(got) == 1 and got[0] == f["jpeg"], "first difference at %d" % first_difference(got[0], f["jpeg"])


def test_a_second_call_a_reversed_batch_and_a_stacked_batch_give_the_same_bytes(eng, batches):
    (q, s, r), names = max(settings().items(), key=lambda kv: len(kv[1]))
    frames = [torch.from_numpy(FIX[n]["bgr"]).cuda() for n in names]
    for _ in range(2):
        assert eng.encode_jpeg_batch(frames, q, s, r) == [batches[n] for n in names]
    assert eng.encode_jpeg_batch(frames[::-1], q, s, r) == [batches[n] for n in reversed(names)]
    f = FIX["long_100x75_444_q100"]
    stack = np.stack([f["bgr"], f["bgr"][::-1].copy(), f["bgr"]])
    got = eng.encode_jpeg_batch(stack, 100, "4:4:4")                   # one (N, H, W, 3) array
    assert got[0] == got[2] == f["jpeg"] and got[1] != f["jpeg"]
    assert eng.encode_jpeg_batch(torch.from_numpy(stack).cuda(), 100, "4:4:4") == got
    assert eng.encode_jpeg_batch([]) == []
    ms = eng.encode_jpeg_batch(stack, 100, "4:4:4", time_iters=2)
    assert len(ms) == 6 and all(m > 0 for m in ms)


def test_the_first_stage_leaves_the_restatements_coefficients_in_the_decoders_layout(eng):
    for (q, s, r), names in settings().items():
        if r:
            continue
        coefs, qt = eng.debug_jpeg_encode_blocks([FIX[n]["bgr"] for n in names], q, s)
        for n, got in zip(names, coefs):
            _, want, want_qt = jen.restated(n)
            assert got.shape == want.shape and int((got != want).sum()) == 0, n
            assert np.array_equal(qt, want_qt), n


def encode_into(eng, frames, caps, quality=75, sampling=2):
    n = len(frames)
    ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in frames])
    heights = (ctypes.c_int * n)(*[f.shape[0] for f in frames])
    widths = (ctypes.c_int * n)(*[f.shape[1] for f in frames])
    outs = [np.full(c, 7, dtype=np.uint8) for c in caps]
    optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    cap = (ctypes.c_size_t * n)(*caps)
    lens = (ctypes.c_size_t * n)()
    rc = _lib.lib().lwp_jpeg_encode_batch(eng.h.ptr, n, ptrs, _lib.MEM_HOST, heights, widths, quality, sampling, 0, optr, cap, lens)
    return rc, _lib.lib().lwp_last_error(eng.h.ptr).decode(), outs, [int(v) for v in lens]


def test_a_capacity_too_small_in_the_middle_fails_the_call_with_its_index_and_writes_nothing(eng):
    names = ["smooth_65x31_420", "restartbig_23x17_420", "noise_50x33_420_q30", "zeros_17x24_420"]
    frames = [FIX[n]["bgr"] for n in names]
    want = eng.encode_jpeg_batch(frames, 75, "4:2:0")
    sizes = [len(w) for w in want]
    rc, msg, outs, _ = encode_into(eng, frames, [sizes[0], sizes[1], sizes[2] - 1, sizes[3]])
    assert rc == _lib.LWP_ERR_CAPACITY and msg.startswith("image 2: ") and str(sizes[2]) in msg, msg
    assert all(bool((o == 7).all()) for o in outs)
    rc, msg, outs, _ = encode_into(eng, frames, [sizes[0], 700, 700, sizes[3]])
    assert rc == _lib.LWP_ERR_CAPACITY and msg.startswith("image 1: "), msg      # the lowest index
    assert all(bool((o == 7).all()) for o in outs)
    rc, msg, outs, lens = encode_into(eng, frames, sizes)                       # exactly enough; and the handle is fine afterwards
    assert rc == _lib.LWP_OK and lens == sizes
    assert [o.tobytes() for o in outs] == want
    with pytest.raises(ValueError, match="image 1: .*1..65535"):
        zero = (ctypes.c_int * 2)(8, 0)
        eng._call("lwp_jpeg_encode_batch", 2, (ctypes.c_void_p * 2)(1, 1), _lib.MEM_HOST, zero, (ctypes.c_int * 2)(8, 8), 75, 2, 0,
                  (ctypes.c_void_p * 2)(), (ctypes.c_size_t * 2)(), (ctypes.c_size_t * 2)())
    for bad in ([np.zeros((4, 4), np.uint8)], [np.zeros((4, 4, 3), np.float32)], [np.zeros((4, 4, 3), np.uint8), torch.zeros(4, 4, 3, dtype=torch.uint8).cuda()],
                np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            eng.encode_jpeg_batch(bad)
    with pytest.raises(ValueError, match="quality"):
        eng.encode_jpeg_batch(frames, quality=0)


def test_a_caller_stream_has_written_the_frames_before_they_are_read(eng):
    f = FIX["long_100x75_444_q100"]
    src = torch.from_numpy(f["bgr"]).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        frames = []
        for _ in range(8):                                               # queued work on the side stream: the frames' producer
            t = torch.zeros_like(src)
            for _ in range(20):
                t = t + 0
            frames.append(t + src)
        got = eng.encode_jpeg_batch(frames, 100, "4:4:4")
    assert got == [f["jpeg"]] * 8


def test_a_closed_engine_has_given_back_what_the_encode_took():
    gc.collect()
    base = live()
    e = Engine(0, nref=1, num_channels=32)
    try:
        created = live()
        names = NAMES[:6]
        got = e.encode_jpeg_batch([FIX[n]["bgr"] for n in names], 75, "4:2:0")
        grown = live()
        assert grown[0] > created[0] and grown[1] > created[1]          # the workspace and the pinned staging are counted
        assert e.encode_jpeg_batch([FIX[n]["bgr"] for n in names], 75, "4:2:0") == got
        assert live() == grown                                          # a second batch of the same size takes nothing more
    finally:
        e.h.close()
    assert live() == base


def test_encode_then_decode_returns_the_restated_decoders_pixels(eng, batches):
    names = [n for n in NAMES if FIX[n]["bgr"].shape[:2] != (1, 1)][::4]
    decoded = eng.decode_jpeg_batch([batches[n] for n in names])
    for n, img in zip(names, decoded):
        want = jc.decode_bgr(FIX[n]["jpeg"])
        assert tuple(img.shape) == FIX[n]["bgr"].shape and int((img.cpu().numpy() != want).sum()) == 0, n


def test_imwrite_then_imread(eng, tmp_path):
    f = FIX["noise_50x33_420_q30"]
    path = str(tmp_path / "out.jpg")
    assert coco.imwrite(path, torch.from_numpy(f["bgr"]).cuda(), eng, quality=30) is True
    with open(path, "rb") as fh:
        assert fh.read() == f["jpeg"]
    assert int((coco.imread(path, eng).cpu().numpy() != jc.decode_bgr(f["jpeg"])).sum()) == 0


@pytest.mark.parametrize("ext", [".avi", ".mjpeg"])
def test_video_writer_then_reader_on_the_card(eng, tmp_path, ext):
    f = FIX["long_100x75_444_q100"]
    frames = [f["bgr"], f["bgr"][:, ::-1].copy(), f["bgr"][::-1].copy(), f["bgr"], f["bgr"][::-1, ::-1].copy()]
    path = str(tmp_path / ("clip" + ext))
    with demo.VideoWriter(path, eng, fps=24, quality=100, subsampling="4:4:4") as vw:
        vw.write(torch.from_numpy(np.stack(frames[:3])).cuda())
        vw.write(frames[3:])
    files = eng.encode_jpeg_batch(frames, 100, "4:4:4")
    assert files[0] == files[3] == f["jpeg"]
    reader = demo.VideoReader(path, eng, batch=2)
    got = list(reader)
    assert len(got) == 5 and all(g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == (75, 100, 3) for g in got)
    for g, data in zip(got, files):
        assert int((g.cpu().numpy() != jc.decode_bgr(data)).sum()) == 0
    if ext == ".avi":
        assert reader.fps == 24
    device = list(demo.VideoReader(path, eng, batch=5, entropy="device"))
    assert all(torch.equal(a, b) for a, b in zip(device, got))


def test_the_reader_decodes_a_hand_built_avi_with_a_frame_without_tables(eng):
    names = ["noise_23x17_420_q100", "checker_23x17_420", "restartbig_23x17_420"]
    files = [FIX[n]["jpeg"] for n in names]
    avi = jen.build_avi([files[0], jen.strip_dht(files[1]), b"", files[2]], 23, 17)
    got = list(demo.VideoReader(avi, eng, batch=3))
    want = [jc.decode_bgr(files[0]), jc.decode_bgr(files[1]), jc.decode_bgr(files[1]), jc.decode_bgr(files[2])]
    assert len(got) == 4 and all(int((g.cpu().numpy() != w).sum()) == 0 for g, w in zip(got, want))


@pytest.fixture(scope="module")
def net():
    n = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(n, {"state_dict": vc.state_dict()})
    return n.eval().cuda(0)


def fields(poses):
    return (np.stack([p.keypoints for p in poses]) if poses else np.zeros((0, 18, 2), np.int32), [p.bbox for p in poses], [p.id for p in poses])


def test_run_demo_fed_by_the_reader_and_the_annotated_frame_kept_on_the_device(net, tmp_path):
    eng = net.engine
    base = vc.pipe_frames("480x640", 2)
    frames = base + [np.roll(base[0], 16, axis=1).copy()]
    path = str(tmp_path / "in.avi")
    with demo.VideoWriter(path, eng, quality=90) as vw:
        vw.write(frames)
    arrays = [t.cpu().numpy() for t in demo.VideoReader(path, eng)]       # what the file holds: the frames after quality 90
    assert len(arrays) == 3 and all(a.shape == (480, 640, 3) for a in arrays)
    runs = {}
    for key, provider, ov in (("arrays", [a.copy() for a in arrays], True), ("reader", demo.VideoReader(path, eng, batch=2), {"device": True})):
        pose_mod.Pose.last_id = -1
        runs[key] = list(demo.run_demo(net, provider, 368, False, True, True, fused=True, device_tail=True, pipelined=True, overlay=ov))
        runs[key + "_last_id"] = pose_mod.Pose.last_id
    pose_mod.Pose.last_id = -1
    assert len(runs["arrays"]) == len(runs["reader"]) == 3 and runs["arrays_last_id"] == runs["reader_last_id"]
    poses = 0
    for t, ((ai, ap), (ri, rp)) in enumerate(zip(runs["arrays"], runs["reader"])):
        fa, fr = fields(ap), fields(rp)
        assert np.array_equal(fa[0], fr[0]) and fa[1:] == fr[1:], t
        assert isinstance(ai, np.ndarray) and ri.is_cuda and ri.dtype == torch.uint8
        assert np.array_equal(ri.cpu().numpy(), ai), t                    # the device-kept annotated frame is the NumPy one
        poses += len(ap)
    assert poses >= 1 and any((runs["arrays"][t][0] != arrays[t]).any() for t in range(3))
    # the serial loop too
    pose_mod.Pose.last_id = -1
    serial = list(demo.run_demo(net, [a.copy() for a in arrays], 368, False, True, True, fused=True, device_tail=True,
                                overlay={"device": True}))
    pose_mod.Pose.last_id = -1
    assert all(s[0].is_cuda and np.array_equal(s[0].cpu().numpy(), a[0]) for s, a in zip(serial, runs["arrays"]))


def test_the_command_line_as_a_fresh_process_writes_the_frames_the_overlay_drew(net, tmp_path, capsys):
    eng = net.engine
    frames = vc.pipe_frames("480x640", 3)
    src, out, ckpt = str(tmp_path / "in.avi"), str(tmp_path / "out.avi"), str(tmp_path / "ckpt.pth")
    with demo.VideoWriter(src, eng, fps=15, quality=90) as vw:
        vw.write(frames)
    torch.save({"state_dict": vc.state_dict()}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = ["--checkpoint-path", ckpt, "--height-size", "368", "--video", src, "--cpu"]
    done = subprocess.run([sys.executable, "-m", "lwpose_amd.demo"] + args + ["--output", out], env=env, cwd=str(tmp_path),
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    reader = demo.VideoReader(out, eng)
    got = list(reader)
    assert len(got) == 3 and reader.fps == 15
    pose_mod.Pose.last_id = -1
    want = list(demo.run_demo(net, demo.VideoReader(src, eng), 368, False, 1, 1, fused=True, device_tail=True, pipelined=True,
                              overlay={"device": True}))
    pose_mod.Pose.last_id = -1
    assert any(len(w[1]) for w in want)
    # the file holds the frames the overlay drew, at the writer's quality 75 (the decoder is pinned in test_gpu_jpeg.py)
    for g, w in zip(got, eng.decode_jpeg_batch(eng.encode_jpeg_batch([w[0] for w in want], 75, "4:2:0"))):
        assert torch.equal(g, w)
    # without --output: one line per frame (index, pose count, ids); the same entry point, in this process
    capsys.readouterr()
    assert demo.main(args) == 0
    pose_mod.Pose.last_id = -1
    rows = [ln.split() for ln in capsys.readouterr().out.strip().splitlines()]
    assert [int(r[0]) for r in rows] == [0, 1, 2] and [int(r[1]) for r in rows] == [len(w[1]) for w in want]
    assert [[int(v) for v in r[2:]] for r in rows] == [[p.id for p in w[1]] for w in want]
