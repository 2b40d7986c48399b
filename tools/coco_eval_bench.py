"""COCO key-point evaluation: the device call against the NumPy restatement of COCOeval, on the same synthetic data sets.

    python tools/coco_eval_bench.py [--images 150 5000] [--iters 50] [--out profiles/eval/coco_eval_bench.json]

A data set is ``--images`` seeded images (tests/coco_eval_cases.Builder) of 1 .. 8 people and 0 .. 15 detections each: jittered
copies of the people and clutter, scores with two decimals.  Records, per data set,
  - its sizes (images, ground truths, detections, selected detections, OKS entries);
  - host time of coco_pack (Python dicts to the packed arrays; what a caller pays once before the device call);
  - wall time of Engine.coco_eval on the packed arrays, best and median of ``--iters`` calls after one warm-up: the upload, the
    three kernels and the sort, the copy back, everything a caller waits for;
  - wall time of the restatement (evaluate + accumulate + summarize) on one CPU core, once;
  - whether the two agree: precision / recall / scores bit for bit, the ten stats."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd.runtime import Engine, coco_pack  # noqa: E402
import coco_eval_cases as cc  # noqa: E402


def make_dataset(n_images, seed):
    b = cc.Builder(seed)
    for i in range(n_images):
        b.image(10 * i + 3, int(b.rng.randint(1, 9)), int(b.rng.randint(0, 16)), crowd=(5,) if i % 9 == 0 else (),
                partly=(0,) if i % 4 == 0 else ())
    return b.done()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[150, 5000])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval", "coco_eval_bench.json"))
    a = ap.parse_args()
    eng = Engine(0)
    runs = []
    for n in a.images:
        gt, dets = make_dataset(n, seed=1000 + n)
        t0 = time.perf_counter()
        packed = coco_pack(gt, dets)
        pack_s = time.perf_counter() - t0
        D, G = np.diff(packed["dt_off"]), np.diff(packed["gt_off"])
        got = eng.coco_eval(packed)
        times = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            got = eng.coco_eval(packed)
            times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ref = cc.reference(gt, dets)
        host_s = time.perf_counter() - t0
        same = all(got[k].tobytes() == np.ascontiguousarray(w).tobytes() for k, w in (
            ("precision", ref.eval["precision"][:, :, 0, :, 0]), ("recall", ref.eval["recall"][:, 0, :, 0]),
            ("scores", ref.eval["scores"][:, :, 0, :, 0])))
        run = {"images": n, "ground_truths": int(G.sum()), "detections": int(D.sum()),
               "selected_detections": int(np.minimum(D, 20).sum()), "oks_entries": int((np.minimum(D, 20) * G).sum()),
               "pack_host_ms": pack_s * 1e3, "device_call_ms_best": min(times) * 1e3, "device_call_ms_median": float(np.median(times)) * 1e3,
               "restatement_host_s": host_s, "arrays_bit_equal": bool(same),
               "stats_device": [float(v) for v in got["stats"]], "stats_restatement": [float(v) for v in ref.stats],
               "speedup_call_vs_restatement": host_s / min(times)}
        print(json.dumps(run), flush=True)
        runs.append(run)
    out = {"tool": "tools/coco_eval_bench.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "runs": runs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
