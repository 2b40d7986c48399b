"""Device-resident validation against the dict route, on the same commit and the same data.

    python tools/val_bench.py [--images 150 5000] [--iters 20] [--frames 48] [--windows 6] [--out profiles/eval/val_bench.json]

Part 1, the evaluation: the synthetic data sets of tools/coco_eval_bench.py.  Both routes start from per-image detection arrays
(key-points (n, 17, 3) and scores (n,), what a detection loop holds after its grouping) and end with the ten stats:
  - dict route: the arrays are turned into ``coco_detections``-shaped dicts, then ``evaluate_detections`` (``coco_pack`` of the
    ground truth and the dicts, one upload, ``lwp_coco_eval``);
  - store route: ``Engine.coco_add_rows`` per image and ``Engine.coco_finish``, with the ground truth resident
    (``coco_pack_gt`` + ``Engine.coco_open`` once, timed separately; ``coco_reset`` before each run is inside the timed span).
Wall time of ``--iters`` runs of each, alternating, best and median; whether the two agree bit for bit.

Part 2, the detection loop: ``--frames`` synthetic frames through a synthetic-weights net at base height 184, once with
``val.coco_detections`` + ``evaluate_detections`` (a synchronise and a fetch per image) and once with ``val.evaluate`` (no host
read in the loop), in ``--windows`` alternating windows after one warm-up of each; best and median window per route, and
whether the stats agree bit for bit.  Printing is redirected; no file is written by either route."""
import argparse
import io
import json
import os
import sys
import time
from contextlib import redirect_stdout

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth, val, workload  # noqa: E402
from lwpose_amd.runtime import Engine, coco_pack, coco_pack_gt  # noqa: E402
from coco_eval_bench import make_dataset  # noqa: E402


def summary(times):
    return {"best_ms": min(times) * 1e3, "median_ms": float(np.median(times)) * 1e3}


def evaluation_runs(eng, n_images, iters):
    gt, dets = make_dataset(n_images, seed=1000 + n_images)
    packed = coco_pack(gt, dets)
    ids = packed["image_ids"]
    per_image = [(packed["dt_kp"][a:b].copy(), packed["dt_score"][a:b].copy()) for a, b in zip(packed["dt_off"][:-1], packed["dt_off"][1:])]

    def dict_route():
        results = []
        for image_id, (kp, sc) in zip(ids, per_image):
            for row, s in zip(kp, sc):
                results.append({'image_id': image_id, 'category_id': 1, 'keypoints': [float(v) for v in row.reshape(-1)], 'score': float(s)})
        with redirect_stdout(io.StringIO()):
            return val.evaluate_detections(gt, results, engine=eng)

    def store_route():
        eng.coco_reset()
        for i, (kp, sc) in enumerate(per_image):
            eng.coco_add_rows(i, kp, sc)
        return eng.coco_finish()["stats"]

    t0 = time.perf_counter()
    eng.coco_open(coco_pack_gt(gt), row_cap=len(dets))
    open_s = time.perf_counter() - t0
    a, b = dict_route(), store_route()                 # warm-up
    td, ts = [], []
    for _ in range(iters):
        t0 = time.perf_counter(); a = dict_route(); td.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b = store_route(); ts.append(time.perf_counter() - t0)
    eng.coco_release()
    return {"images": n_images, "detections": len(dets), "ground_truths": int(packed["gt_off"][-1]),
            "open_ms_once": open_s * 1e3, "dict_route": summary(td), "store_route": summary(ts),
            "stats_bit_equal": bool(np.asarray(a).tobytes() == np.asarray(b).tobytes()),
            "dict_over_store_best": min(td) / min(ts)}


def loop_runs(n_frames, windows):
    net, _ = workload.build_net(nref=1, seed=1, device=0, height=184, width=328, multiscale=[1])
    samples = [{"file_name": "%012d.jpg" % (100 + 3 * i), "img": synth.make_frames(1, 184, 328, seed0=i)[0]} for i in range(n_frames)]
    results = val.coco_detections(net, samples, multiscale=False, base_height=184)
    anns = []
    for n, r in enumerate(results[::2]):
        kp = np.array(r["keypoints"]).reshape(17, 3)
        vis = kp[:, 2] > 0
        xy = kp[vis, :2]
        w, h = float(np.ptp(xy[:, 0])), float(np.ptp(xy[:, 1]))
        kp[vis, 2] = 2
        anns.append({"id": n + 1, "image_id": r["image_id"], "category_id": 1, "keypoints": kp.reshape(-1).tolist(),
                     "num_keypoints": int(vis.sum()), "area": max(w * h, 1.0), "iscrowd": 0,
                     "bbox": [float(xy[:, 0].min()), float(xy[:, 1].min()), w, h]})
    gt = {"images": [{"id": 100 + 3 * i} for i in range(n_frames)], "annotations": anns, "categories": [{"id": 1, "name": "person"}]}

    def dict_route():
        with redirect_stdout(io.StringIO()):
            return val.evaluate_detections(gt, val.coco_detections(net, samples, multiscale=False, base_height=184), engine=net.engine)

    def store_route():
        with redirect_stdout(io.StringIO()):
            return val.evaluate(gt, None, samples, net, multiscale=False, store=True, base_height=184)

    a, b = dict_route(), store_route()                 # warm-up
    td, ts = [], []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); a = dict_route(); td.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); b = store_route(); ts.append(time.perf_counter() - t0)
    net.engine.coco_release()
    return {"frames": n_frames, "frame_size": [184, 328], "detections": len(results), "windows": windows,
            "dict_route": summary(td), "store_route": summary(ts),
            "dict_route_ms_per_frame_best": min(td) * 1e3 / n_frames, "store_route_ms_per_frame_best": min(ts) * 1e3 / n_frames,
            "stats_bit_equal": bool(np.asarray(a).tobytes() == np.asarray(b).tobytes()), "dict_over_store_best": min(td) / min(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[150, 5000])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "val_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    runs = []
    for n in a.images:
        run = evaluation_runs(eng, n, a.iters)
        print(json.dumps(run), flush=True)
        runs.append(run)
    loop = loop_runs(a.frames, a.windows)
    print(json.dumps(loop), flush=True)
    out = {"tool": "tools/val_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "evaluation": runs, "detection_loop": loop}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
