"""Crowd masks: rendered on the device from RLE runs against decoded on the host and uploaded as float masks.

    python tools/crowd_mask_bench.py [--batch 80] [--crop 368] [--iters 50] [--out profiles/train/crowd_mask_bench.json]

The training shape of tools/augment_bench.py: batch 80, 480 x 640 sources, crop 368 x 368, the reference's default transform
parameters.  Every sample carries two crowd RLEs of about a thousand runs each (unions of discs).  Records
  - kernel time of the crowd-mask kernel alone (lwp_time_crowd_masks: HIP events around 20 x ``iters`` back-to-back launches
    after one upload and a warm-up; three such windows, the median);
  - the time of a whole Engine.augment_batch call from host images + segmentations (lwp_augment_batch_crowd: packing, the one
    upload, both kernels, synchronise), ``iters`` calls a window, three windows alternating with the next route, the median;
  - the same call on the existing route: host images + float masks that NumPy decoded beforehand (lwp_augment_batch), and the
    host time of that decode (datasets.coco.get_mask), which the existing route pays as well;
  - the bytes each route uploads."""
import argparse
import ctypes
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd._lib import AugmentPlan  # noqa: E402
from lwpose_amd.datasets import coco  # noqa: E402
from lwpose_amd.datasets import transformations as T  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402
import augment_cases as ac  # noqa: E402


def encode(grid):
    """Boolean (h, w) grid -> uncompressed RLE dict (column-major runs that start with zeros)."""
    flat = grid.reshape(-1, order="F")
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    counts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
    return {"counts": ([0] if flat[0] else []) + counts, "size": [int(grid.shape[0]), int(grid.shape[1])]}


def discs(h, w, seed, n=5):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    grid = np.zeros((h, w), dtype=bool)
    for _ in range(n):
        cy, cx, r = g.uniform(0, h), g.uniform(0, w), g.uniform(40, 70)
        grid |= (y - cy) ** 2 + (x - cx) ** 2 < r * r
    return grid


def call_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def pad16(n):
    return (n + 15) & ~15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--crop", type=int, default=368)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "crowd_mask_bench.json"))
    a = ap.parse_args()
    N, S, H, W = a.batch, a.crop, 480, 640
    pad = (128, 128, 128)
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=pad), T.CropPad(pad=pad, crop_x=S, crop_y=S), T.Flip()]
    provided = np.linspace(0.1, 1.0, N)
    with_segs, with_masks, runs = [], [], []
    decode_s = 0.0
    for n in range(N):
        s = ac.synthetic_sample(n, H, W, others=n % 3, scale_provided=float(provided[n]), with_mask=False)
        del s["mask"]
        segs = [encode(discs(H, W, 2 * n)), encode(discs(H, W, 2 * n + 1))]
        runs += [len(seg["counts"]) for seg in segs]
        t0 = time.perf_counter()
        mask = coco.get_mask(segs, np.ones((H, W), dtype=np.float32))
        decode_s += time.perf_counter() - t0
        with_segs.append(dict(s, segmentations=segs))
        with_masks.append(dict(s, mask=mask))
    out = {"workload": "batch %d, %dx%d sources, crop %dx%d, two crowd RLEs a sample" % (N, H, W, S, S), "iters": a.iters,
           "runs_per_rle_min_mean_max": [int(min(runs)), float(np.mean(runs)), int(max(runs))],
           "numpy_get_mask_ms_per_batch": decode_s * 1e3}

    eng = Engine(0, nref=1, num_channels=32)           # neither call needs weights
    segs_per_image, sizes = [s["segmentations"] for s in with_segs], [(H, W)] * N
    eng.crowd_masks(segs_per_image, sizes, time_iters=2)
    k = 20 * a.iters                                   # a launch takes tens of microseconds: a window of its own length
    out["kernel_launches_timed"] = k
    out["kernel_ms_runs"] = [eng.crowd_masks(segs_per_image, sizes, time_iters=k) / k for _ in range(3)]
    out["kernel_ms"] = float(np.median(out["kernel_ms_runs"]))
    out["kernel_bytes_written"] = N * H * W * 4
    plan_segs = T.plan_batch(with_segs, transforms, random.Random(0))
    plan_masks = T.plan_batch(with_masks, transforms, random.Random(0))
    a_ms, b_ms = [], []
    for _ in range(3):                                 # the two routes in turn, so that a busy host shows in both
        a_ms.append(call_ms(lambda: eng.augment_batch(plan_segs), a.iters))
        b_ms.append(call_ms(lambda: eng.augment_batch(plan_masks), a.iters))
    out["call_ms_runs_host_images_and_segmentations"], out["call_ms_runs_host_images_and_float_masks"] = a_ms, b_ms
    out["call_ms_host_images_and_segmentations"] = float(np.median(a_ms))
    out["call_ms_host_images_and_float_masks"] = float(np.median(b_ms))
    got, want = eng.augment_batch(plan_segs), eng.augment_batch(plan_masks)
    out["elements_differing_between_the_routes"] = int(sum(int((g != w).sum()) for g, w in zip(got[:3], want[:3])))

    counts, seg_off, image_seg_off = coco.pack_crowd_runs(segs_per_image, sizes)
    records = pad16(N * ctypes.sizeof(AugmentPlan))
    tables = pad16(4 * len(counts)) + pad16(4 * len(seg_off)) + pad16(24 * N)     # run ends, segment offsets (uint32), image records
    out["upload_bytes_segmentations"] = records + N * pad16(H * W * 3) + tables
    out["upload_bytes_float_masks"] = records + N * (pad16(H * W * 3) + pad16(H * W * 4))
    out["run_table_bytes"] = tables
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
