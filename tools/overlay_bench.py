"""Pose overlay: the host cost of drawing against the device kernels, and the run_demo loop with each.

    python tools/overlay_bench.py [--frames 60] [--rounds 3] [--out profiles/overlay/overlay_bench.json]
    rocprofv3 --kernel-trace --stats -d DIR -o ov -- python tools/overlay_bench.py --kernels-only     (a run of its own)
    python tools/overlay_bench.py --merge-kernel-stats DIR        (adds the overlay kernels' device time from that run's *kernel_stats.csv)

The tracking bench's setting: 720x1280 uint8 frames, batch 1, and for the drawing cost the pose rows of the 35-pose crowd fixture
(tests/golden/tail_crowd35.npz, frame 0).  Records per frame: the host time of the parent's draw=True path (Pose.draw over the
poses), the same plus a NumPy blend and boxes, the wall time of Engine.draw_poses (device frame in and out, pose upload and
synchronise included), and the pipelined run_demo loop rate with overlay=True, with draw=True and without drawing."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import demo, synth, workload  # noqa: E402
from lwpose_amd.modules.pose import Pose  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

KERNELS = ("overlay_copy_kernel", "overlay_copy_bytes_kernel", "overlay_stamps_kernel", "overlay_boxes_kernel")


def crowd():
    z = np.load(os.path.join(ROOT, "tests", "golden", "tail_crowd35.npz"))
    n = int(z["crowd35_plain:n"][0])
    return z["crowd35_plain:out_kp"][:n].copy(), z["crowd35_plain:out_bbox"][:n].copy()


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [float(x) for x in v]}


def host_draw(frame, kp, bbox, blend):
    t0 = time.perf_counter()
    img = frame.copy() if blend else frame
    for k in kp:
        Pose(k, 1.0).draw(img)
    if blend:                                            # demo.py:120-124 in NumPy
        img = ((6 * frame.astype(np.uint16) + 4 * img.astype(np.uint16) + 5) // 10).astype(np.uint8)
        h, w = frame.shape[:2]
        for x, y, bw, bh in bbox.tolist():
            xs, ys = slice(max(x, 0), max(min(x + bw, w - 1) + 1, 0)), slice(max(y, 0), max(min(y + bh, h - 1) + 1, 0))
            for yy in (y, y + bh):
                if 0 <= yy < h:
                    img[yy, xs] = (0, 255, 0)
            for xx in (x, x + bw):
                if 0 <= xx < w:
                    img[ys, xx] = (0, 255, 0)
    return time.perf_counter() - t0


def loop_fps(net, frames, **kw):
    Pose.last_id = -1
    t0 = time.perf_counter()
    n = sum(len(p) for _, p in demo.run_demo(net, [f.copy() for f in frames], 368, False, True, False, fused=True, device_tail=True,
                                             pipelined=True, **kw))
    return len(frames) / (time.perf_counter() - t0), n / len(frames)


def merge(out_path, stats_dir):
    with open(out_path) as f:
        out = json.load(f)
    rows = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0].split("::")[-1]
            if name in KERNELS:
                rows[name] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    out["device_kernels_rocprofv3"] = dict(rows, sum_of_averages_us=sum(v["average_us"] for v in rows.values()))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["device_kernels_rocprofv3"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--merge-kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay", "overlay_bench.json"))
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge(a.out, a.merge_kernel_stats)
    kp, bbox = crowd()
    frame = synth.make_frames(1, 720, 1280, seed0=0)[0]
    if a.kernels_only:                                   # what a rocprofv3 --kernel-trace run measures
        eng = Engine(0)
        d = torch.from_numpy(frame).cuda(0)
        for _ in range(50):
            eng.draw_poses(d, kp, bbox)
        eng.synchronize()
        return
    out = {"workload": "720x1280 uint8 frame, %d poses of tests/golden/tail_crowd35.npz, batch 1" % len(kp), "poses": len(kp)}
    out["host_pose_draw_ms"] = stats([host_draw(frame.copy(), kp, bbox, False) * 1e3 for _ in range(a.rounds)])
    out["host_pose_draw_blend_boxes_ms"] = stats([host_draw(frame.copy(), kp, bbox, True) * 1e3 for _ in range(a.rounds)])
    eng = Engine(0)
    d = torch.from_numpy(frame).cuda(0)
    eng.draw_poses(d, kp, bbox)
    ts = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100):
            o = eng.draw_poses(d, kp, bbox)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 10)
    out["engine_draw_poses_call_ms"] = stats(ts)
    del o
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    base = synth.make_frames(1, 720, 1280, seed0=0)[0]
    frames = [np.ascontiguousarray(np.roll(base, 16 * t, axis=1)) for t in range(a.frames)]
    loops = {"none": dict(), "draw": dict(draw=True), "overlay": dict(overlay=True)}
    for kw in loops.values():
        loop_fps(net, frames[:6], **kw)
    fps = {k: [] for k in loops}
    poses = 0.0
    for _ in range(a.rounds):                            # alternating
        for k, kw in loops.items():
            f, poses = loop_fps(net, frames, **kw)
            fps[k].append(f)
    out["run_demo_pipelined_fps"] = dict({k: stats(v) for k, v in fps.items()}, poses_per_frame=poses, frames=a.frames)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
