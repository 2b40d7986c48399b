"""The video loop: serial device tail against the one-call pipelined step, camera batches, and the batched pre-processing kernel.

    python tools/video_bench.py [--frames 60] [--rounds 5] [--parent-root DIR] [--out profiles/video/video_bench.json]

(a) run_demo loop, frames/s: ``fused=True, device_tail=True`` (serial: five C calls per frame) against the same with
    ``pipelined=True`` (lwp_pipeline_submit_u8, frame k + 1 submitted before frame k is fetched).  The frames are
    tools/track_bench.py's: 720x1280 uint8, height 368, track on, smoothing off and on.  Every measurement is a fresh child
    process (so a tree without the new exports can take part); the children ALTERNATE: parent-tree serial (if ``--parent-root``
    names a built checkout of the parent commit), this tree serial, this tree pipelined, ``--rounds`` times.  Medians, min, max.
(b) run_cameras (TRACK_LANES, pipelined) at 4 and 32 streams, frames/s over all streams.
(c) device time of the batched kernel against N launches of the single-frame kernel — a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats -d DIR -o kern -- python tools/video_bench.py --kernel-run 4
    python tools/video_bench.py --kernel-stats DIR --kernel-n 4 [--out ...]     # folds the stats into the JSON

    ``--kernel-run N`` launches, on frames already in device memory, R x the batched kernel in its four-pixel form, R x in its
    one-pixel form and R x N x the single-frame kernel.
(d) the bench.py headline of this tree against the parent's, alternating (the default path is untouched: expected equal):

    python tools/video_bench.py --headline --parent-root DIR [--rounds 5] [--out ...]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": [float(x) for x in v]}


def bench_frames(n):
    from lwpose_amd import synth
    base = synth.make_frames(1, 720, 1280, seed0=0)[0]
    return [np.ascontiguousarray(np.roll(base, 16 * t, axis=1)) for t in range(n)]


# ------------------------------------------------------------------------------------------ children (one measurement each)
def child_loop(a):
    """One process, one tree (sys.path[0] is its root): frames/s of the run_demo loop, plain and smoothed —
    one warm-up pass of 8 frames, then ``--reps`` timed passes whose median is reported."""
    from lwpose_amd import demo, workload
    from lwpose_amd.modules.pose import Pose
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    frames = bench_frames(a.frames)
    kw = dict(fused=True, device_tail=True)
    if a.child == "pipelined":
        kw["pipelined"] = True
    out = {}
    for smooth in (False, True):
        def one(fr):
            Pose.last_id = -1
            n = 0
            t0 = time.perf_counter()
            for _, poses in demo.run_demo(net, fr, 368, False, True, smooth, **kw):
                n += len(poses)
            return len(fr) / (time.perf_counter() - t0), n / len(fr)
        one(frames[:8])
        runs = [one(frames) for _ in range(a.reps)]
        out["smooth" if smooth else "plain"] = {"fps": float(np.median([r[0] for r in runs])), "poses_per_frame": runs[0][1]}
    print("RESULT " + json.dumps(out))


def child_cameras(a):
    from lwpose_amd import demo, workload
    from lwpose_amd.modules.pose import Pose
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    frames = bench_frames(a.frames)
    out = {}
    for n in (4, 32):
        steps = max(4, a.frames // n * 4)
        provs = [[frames[(t + 3 * l) % len(frames)] for t in range(steps)] for l in range(n)]

        def one():
            Pose.last_id = -1
            t0 = time.perf_counter()
            k = sum(1 for _ in demo.run_cameras(net, provs, 368, True, True))
            return k * n / (time.perf_counter() - t0)
        one()
        out["streams%d" % n] = stats([one() for _ in range(a.reps)])
        out["streams%d" % n]["steps"] = steps
    print("RESULT " + json.dumps(out))


def child_kernels(a):
    """Launches only (to be run under the profiler): device-resident frames, no uploads."""
    import torch
    from lwpose_amd.runtime import Engine
    n, reps = a.kernel_run, a.reps * 40
    frames = torch.from_numpy(np.stack(bench_frames(n))).cuda()
    engines = {}
    for vec in ("1", "0"):
        os.environ["LWP_PRE_BATCH_VEC"] = vec
        engines[vec] = Engine(0)
    for vec, eng in engines.items():
        for _ in range(reps):
            eng.preprocess_u8_batch(frames, 368, 8)
        eng.synchronize()
    eng = engines["1"]
    for _ in range(reps):
        for f in range(n):
            eng.preprocess_u8(frames[f], 368, 8)
    eng.synchronize()
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"N": n, "reps": reps}))


def run_child(root, mode, a, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--root", root, "--frames", str(a.frames), "--reps", str(a.reps)] + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("child %s in %s failed (%d):\n%s" % (mode, root, p.returncode, p.stderr[-2000:]))
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def headline(a):
    """bench.py --gpus 1 of the parent tree and of this one, alternating, ``--rounds`` fresh processes each."""
    trees = [("parent", os.path.abspath(a.parent_root)), ("this", HERE)]
    runs = {label: [] for label, _ in trees}
    for _ in range(a.rounds):
        for label, root in trees:
            p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "10"],
                               cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError("bench.py in %s failed (%d):\n%s" % (root, p.returncode, p.stderr[-2000:]))
            line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
            runs[label].append(json.loads(line)["value"])
    out = {label + "_fps": stats(v) for label, v in runs.items()}
    out["this_over_parent_medians"] = float(np.median(runs["this"]) / np.median(runs["parent"]))
    out["protocol"] = "bench.py --gpus 1 --steps 200 --warmup 10, one fresh process per figure, parent / this alternating, %d rounds" % a.rounds
    return out


# ------------------------------------------------------------------------------------------ profiler stats -> JSON
def kernel_stats(a):
    files = sorted(glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % a.kernel_stats)
    rows = {}
    for r in csv.DictReader(open(files[-1])):
        name = r.get("Name") or r.get("KernelName") or ""
        if "preprocess_u8" in name:
            rows[name] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                          "max_us": float(r["MaxNs"]) / 1e3, "stddev_us": float(r.get("StdDev", 0) or 0) / 1e3}
    n = a.kernel_n
    out = {"N": n, "kernels": rows}
    single = [v for k, v in rows.items() if "batch" not in k]
    if single:
        out["single_frame_x_N_us"] = single[0]["average_us"] * n
    for k, v in rows.items():
        if "batch" in k:
            out["batched_%s_us" % ("px4" if "<4>" in k else "px1")] = v["average_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "video", "video_bench.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--kernel-run", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--kernel-n", type=int, default=4)
    ap.add_argument("--headline", action="store_true")
    a = ap.parse_args()
    if a.child or a.kernel_run:
        sys.path.insert(0, os.path.abspath(a.root))
        import lwpose_amd  # noqa: F401
        if a.kernel_run:
            return child_kernels(a)
        return child_cameras(a) if a.child == "cameras" else child_loop(a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.headline:
        if not a.parent_root:
            raise SystemExit("--headline needs --parent-root")
        out["bench_headline"] = headline(a)
    elif a.kernel_stats:
        out.setdefault("preprocess_kernel_device_time", {})["N%d" % a.kernel_n] = kernel_stats(a)
    else:
        trees = ([("parent_serial", os.path.abspath(a.parent_root), "serial")] if a.parent_root else []) + \
                [("serial", HERE, "serial"), ("pipelined", HERE, "pipelined")]
        runs = {label: {"plain": [], "smooth": []} for label, _, _ in trees}
        poses = 0.0
        for _ in range(a.rounds):                          # alternating, one fresh process each
            for label, root, mode in trees:
                r = run_child(root, mode, a)
                for k in ("plain", "smooth"):
                    runs[label][k].append(r[k]["fps"])
                poses = r["plain"]["poses_per_frame"]
        loop = {"poses_per_frame": poses}
        for k in ("plain", "smooth"):
            loop[k] = {label + "_fps": stats(v[k]) for label, v in runs.items()}
            base = "parent_serial" if a.parent_root else "serial"
            loop[k]["pipelined_over_%s_medians" % base] = float(np.median(runs["pipelined"][k]) / np.median(runs[base][k]))
        out.update({"workload": "720x1280 uint8 frames -> height 368 (368x656 network input), nref 1, fp32, fused, device tail, track=True",
                    "protocol": "every figure is one child process (build, 8 warm-up frames, median of %d passes over %d frames); the children "
                                "alternate %s, %d rounds; medians, min and max over the rounds" % (a.reps, a.frames, " / ".join(t[0] for t in trees), a.rounds),
                    "frames": a.frames, "rounds": a.rounds, "run_demo": loop, "run_cameras_fps": run_child(HERE, "cameras", a)})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
