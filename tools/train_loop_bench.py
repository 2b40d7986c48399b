"""``train.train`` with the loss log on the device against the same loop fetching the losses every step.

    python tools/train_loop_bench.py [--batch 80] [--iters 12] [--warm 3] [--windows 3] [--scope all]
                                     [--out profiles/train/train_loop_bench.json]

Workload: a temporary folder of ``batch`` generated JPEG files of 480 x 640 (4:2:0, quality 90, textured synthetic content,
made with Pillow; without Pillow the tool records that and quotes no figure) under ``(warm + iters + 1) * batch`` synthetic labels
of two persons and one crowd RLE each (every file is listed that often, so a window stays inside one epoch and meets no
epoch-top reset of the log), trained at the reference's shape (368 x 368 crops, one refinement stage, batches_per_iter 1).  Both routes are
``train(..., max_iters=warm + iters)`` of this commit, in alternating windows; the fetching route replaces the loop's step by
the same ``val.augmented_train_step`` with ``log=False`` (the losses are copied to the host and the stream is waited for in
every step, as before the log existed).  A window's clock starts when step ``warm + 1`` begins and stops when ``train`` returns,
behind the ``read_loss_log`` of the last iteration (log_after = warm + iters), which waits for the stream: the rate is
iterations over a wall time that ends in a device synchronise.  No ratio is fixed in advance."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import train as train_mod  # noqa: E402
from lwpose_amd import val  # noqa: E402


def make_folder(folder, files, count, H, W):
    from PIL import Image
    from jpeg_bench import textured
    g = np.random.default_rng(0)
    labels = []
    for n in range(files):
        Image.fromarray(textured(H, W, n)).save(os.path.join(folder, "%06d.jpg" % n), "JPEG", quality=90, subsampling=2)
    for n in range(count):
        name = "%06d.jpg" % (n % files)

        def person():
            kps = [[float(g.uniform(0, W)), float(g.uniform(0, H)), int(g.integers(0, 2))] for _ in range(17)]
            return {"keypoints": kps, "objpos": [float(g.uniform(0.35, 0.65) * W), float(g.uniform(0.35, 0.65) * H)], "scale_provided": 0.6}
        label = person()
        runs = [H * 100 + 100] + [200, H - 200] * 20                   # column-major runs: a 200 x 20 block of crowd
        label.update(img_paths=name, img_width=W, img_height=H, processed_other_annotations=[person()],
                     segmentations=[{"size": [H, W], "counts": runs}])
        labels.append(label)
    return labels


def window(labels, folder, a, fetch):
    stamps = []
    step = val.augmented_train_step

    def timed(net, opt, samples, augment, batches_per_iter=1, sigma=7, paf_thickness=1, log=False):
        stamps.append(time.perf_counter())
        return step(net, opt, samples, augment, batches_per_iter, sigma, paf_thickness, log=log and not fetch)
    train_mod.augmented_train_step = timed
    total = a.warm + a.iters
    try:
        with contextlib.redirect_stdout(io.StringIO()), tempfile.TemporaryDirectory() as ck:
            train_mod.train(labels, folder, 1, 4e-5, a.batch, 1, 0, None, False, False, ck, total, None, None, None, 10 ** 9, 10 ** 9,
                            scope=a.scope, max_iters=total, seed=1)
            end = time.perf_counter()
    finally:
        train_mod.augmented_train_step = step
    assert len(stamps) == total
    return a.iters / (end - stamps[a.warm])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--scope", default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "train_loop_bench.json"))
    a = ap.parse_args()
    out = {"workload": "batch %d of 480x640 4:2:0 JPEG files, 368x368 crops, nref 1, scope %s, batches_per_iter 1; %d warm + %d timed "
                       "iterations a window" % (a.batch, a.scope, a.warm, a.iters)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    try:
        import PIL  # noqa: F401
    except ImportError:
        out["pillow"] = "absent: no input files, no figure"
    else:
        with tempfile.TemporaryDirectory() as folder:
            labels = make_folder(folder, a.batch, (a.warm + a.iters + 1) * a.batch, 480, 640)
            logged, fetched = [], []
            for _ in range(a.windows):
                logged.append(window(labels, folder, a, fetch=False))
                fetched.append(window(labels, folder, a, fetch=True))
        out["iterations_per_s_device_log_runs"], out["iterations_per_s_fetch_every_step_runs"] = logged, fetched
        out["iterations_per_s_device_log"] = float(np.median(logged))
        out["iterations_per_s_fetch_every_step"] = float(np.median(fetched))
        out["ms_per_iteration_device_log"] = 1e3 / out["iterations_per_s_device_log"]
        out["ms_per_iteration_fetch_every_step"] = 1e3 / out["iterations_per_s_fetch_every_step"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
