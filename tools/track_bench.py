"""run_demo loop with tracking: Python tail (device_tail=False, the parent's code path) against the device pose tail.

    python tools/track_bench.py [--frames 60] [--rounds 5] [--out profiles/tracking/track_bench.json]

Calibrated 368x656 workload (720x1280 uint8 frames, height_size 368), batch 1, fused=True, track=True, smooth on and off; the
two tails alternate in one process, medians and spread over the rounds.  Also: batch 32 in sequence mode (one
lwp_infer_poses call per 32 frames, poses read with Engine.poses) and the device time of the tail's two launches next to the
rest of the post chain (lwp_profile_launches, post class, one run)."""
import argparse
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


def demo_fps(net, frames, smooth, device_tail):
    Pose.last_id = -1
    n = 0
    t0 = time.perf_counter()
    for _, poses in demo.run_demo(net, frames, 368, False, True, smooth, fused=True, device_tail=device_tail):
        n += len(poses)
    return len(frames) / (time.perf_counter() - t0), n / len(frames)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracking", "track_bench.json"))
    a = ap.parse_args()
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    base = synth.make_frames(1, 720, 1280, seed0=0)[0]
    frames = [np.ascontiguousarray(np.roll(base, 16 * t, axis=1)) for t in range(a.frames)]
    out = {"workload": "720x1280 uint8 frames -> height 368 (368x656 network input), nref 1, fp32, batch 1, fused, track=True",
           "frames": a.frames, "rounds": a.rounds, "run_demo": {}}
    for smooth in (False, True):
        demo_fps(net, frames[:8], smooth, False)
        demo_fps(net, frames[:8], smooth, True)
        py, dev, poses = [], [], 0.0
        for _ in range(a.rounds):                      # alternating
            f, poses = demo_fps(net, frames, smooth, False)
            py.append(f)
            dev.append(demo_fps(net, frames, smooth, True)[0])
        out["run_demo"]["smooth" if smooth else "plain"] = {"poses_per_frame": poses, "python_tail_fps": stats(py), "device_tail_fps": stats(dev),
                                                            "speedup_of_medians": float(np.median(dev) / np.median(py))}
    # batch 32, sequence mode: the network-normalised frames stay on the device
    eng = net.engine
    x = torch.from_numpy(workload.normalized_input(np.stack([np.roll(synth.make_frames(1, 368, 656, seed0=0)[0], 8 * t, axis=1) for t in range(32)]))).cuda()
    seq = {}
    for mode, label in ((eng.TRACK_OFF, "tail_off"), (eng.TRACK_SEQUENCE, "sequence_smooth")):
        eng.set_tracking(mode, smooth=True)
        ts = []
        for r in range(a.rounds + 1):
            t0 = time.perf_counter()
            eng.infer_poses(x, 4, True)
            if mode:
                eng.poses()
            ts.append(32 / (time.perf_counter() - t0))
        seq[label] = stats(ts[1:])
    out["batch32_infer_poses_fps"] = seq
    # device time of the launches, one run (post class): the tail next to the rest of the chain
    prof = {}
    for n in (1, 32):
        eng.set_tracking(eng.TRACK_SEQUENCE, smooth=True)
        eng.infer_poses(x[:n].contiguous(), 4, True)            # a previous frame to match against
        pl = eng.profile_launches(x[:n].contiguous(), reps=20)
        post = [(name, ms) for name, k, ms in pl if k == 4]
        prof["batch%d" % n] = {"post_launches_us": {name: round(ms * 1e3, 2) for name, ms in post},
                               "post_chain_without_tail_us": round(sum(ms for name, ms in post if not name.startswith("tail_")) * 1e3, 2),
                               "tail_us": round(sum(ms for name, ms in post if name.startswith("tail_")) * 1e3, 2),
                               "all_launches_us": round(sum(ms for _, _, ms in pl) * 1e3, 2)}
    eng.set_tracking(eng.TRACK_OFF)
    out["device_time"] = prof
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
