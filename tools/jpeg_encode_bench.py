"""The JPEG encoder measured; nothing is fixed in advance.

    python tools/jpeg_encode_bench.py [--batch 8] [--iters 10] [--out profiles/video/jpeg_encode_bench.json]

Workload: ``batch`` frames of 720 x 1280 from synth.make_frames (low-frequency content plus fine noise), 4:2:0, quality 75.  Records
  - the six stages' device time by HIP events around back-to-back launches (lwp_time_jpeg_encode_batch), three windows, the
    median per stage;
  - the whole encode_jpeg_batch call from device frames against "download the frames, Pillow on 16 threads", alternating
    windows on this commit; without Pillow the tool says so and quotes no figure for that leg;
  - the bytes that cross PCIe both ways: compressed files against raw frames;
  - the pipelined demo loop (run_demo(fused, device_tail, pipelined, overlay)) with the annotated frame fetched as a NumPy array
    and dropped, against the same loop with the frame kept on the device and written by VideoWriter, alternating."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import demo, synth  # noqa: E402
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet  # noqa: E402
from lwpose_amd.modules import pose as pose_mod  # noqa: E402
from lwpose_amd.modules.load_state import load_state  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

STAGES = ["A colour, sampling, DCT, quantiser", "B bit counts", "C offsets", "D memset and code write", "E FF counts", "F stuffing"]


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--demo-frames", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video", "jpeg_encode_bench.json"))
    a = ap.parse_args()
    N, H, W = a.batch, 720, 1280
    out = {"workload": "batch %d, %dx%d, synth.make_frames, 4:2:0, quality 75" % (N, H, W), "iters": a.iters,
           "device": torch.cuda.get_device_name(0)}
    eng = Engine(0, nref=1, num_channels=32)
    host = synth.make_frames(N, H, W)
    dev = torch.from_numpy(host).cuda()
    files = eng.encode_jpeg_batch(dev)
    out["file_bytes_per_frame"] = sum(map(len, files)) / N
    out["raw_bytes_per_frame"] = H * W * 3
    out["pcie_ratio_raw_over_compressed"] = H * W * 3 * N / sum(map(len, files))
    windows = [eng.encode_jpeg_batch(dev, time_iters=a.iters) for _ in range(3)]
    out["stage_ms_per_batch"] = {s: statistics.median(w[k] for w in windows) / a.iters for k, s in enumerate(STAGES)}
    out["stages_ms_per_batch_sum"] = sum(out["stage_ms_per_batch"].values())
    try:
        from PIL import Image
    except ImportError:
        Image = None
        out["pillow"] = "absent: the host leg was not run"
    pool = ThreadPoolExecutor(16)

    def pillow_leg():
        frames = dev.cpu().numpy()

        def one(f):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(buf, "JPEG", quality=75, subsampling=2)
            return buf.getvalue()
        return list(pool.map(one, frames))

    dev_ms, pil_ms = [], []
    for _ in range(3):
        dev_ms.append(wall_ms(lambda: eng.encode_jpeg_batch(dev), a.iters))
        if Image is not None:
            pil_ms.append(wall_ms(pillow_leg, max(a.iters // 2, 1)))
    out["encode_jpeg_batch_ms_per_batch"] = {"windows": dev_ms, "median": statistics.median(dev_ms)}
    if Image is not None:
        out["download_plus_pillow_16_threads_ms_per_batch"] = {"windows": pil_ms, "median": statistics.median(pil_ms)}
        out["same_bytes_as_pillow"] = pillow_leg() == files
    # the pipelined demo loop with and without the writer
    import video_cases as vc
    net = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(net, {"state_dict": vc.state_dict()})
    net = net.eval().cuda(0)
    frames = [np.ascontiguousarray(f) for f in synth.make_frames(a.demo_frames, H, W)]

    def loop(write):
        pose_mod.Pose.last_id = -1
        t0 = time.perf_counter()
        if write:
            with tempfile.TemporaryDirectory() as d, demo.VideoWriter(os.path.join(d, "out.avi"), net) as vw:
                for img, _ in demo.run_demo(net, frames, 368, False, True, True, fused=True, device_tail=True, pipelined=True,
                                            overlay={"device": True}):
                    vw.write(img)
        else:
            for img, _ in demo.run_demo(net, frames, 368, False, True, True, fused=True, device_tail=True, pipelined=True, overlay=True):
                pass
        return (time.perf_counter() - t0) * 1e3 / len(frames)

    loop(False), loop(True)
    plain, written = [], []
    for _ in range(3):
        plain.append(loop(False))
        written.append(loop(True))
    out["demo_loop_ms_per_frame"] = {"annotated frame to a NumPy array, dropped": {"windows": plain, "median": statistics.median(plain)},
                                     "annotated frame kept on the device, VideoWriter": {"windows": written, "median": statistics.median(written)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
