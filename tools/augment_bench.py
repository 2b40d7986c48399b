"""Training augmentation: the device kernel against the staged NumPy route, and its share of a training step.

    python tools/augment_bench.py [--batch 80] [--crop 368] [--iters 50] [--out profiles/train/augment_bench.json]

The reference's training shape: batch 80, 480 x 640 sources, crop 368 x 368, ``scale_provided`` spread evenly over 0.1 .. 1.0
(so the resize enlarges by 0.3 x .. 6.6 x), the reference's default transform parameters.  Records
  - kernel time of the augmentation (lwp_time_augment_batch: HIP events around ``iters`` back-to-back launch pairs after one
    upload and a warm-up) with the sources resident in device memory, and the time of a whole Engine.augment_batch call with
    device sources and with host sources (packing, the one upload, launch, synchronise: what a caller waits for);
  - host time of plan_batch (the random draws and the label arithmetic of the batch);
  - host time of the staged NumPy route (resize, warp, crop, flip as full images) on ``--host-samples`` samples spread over
    the scale range, scaled to the batch;
  - time of val.train_step (unchanged by the augmentation) at the same batch and crop on an fp32 nref-1 net, so the
    augmentation's share of a step is known."""
import argparse
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
from lwpose_amd import optim, synth, val  # noqa: E402
from lwpose_amd.datasets import transformations as T  # noqa: E402
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet  # noqa: E402
from lwpose_amd.modules.load_state import load_state  # noqa: E402
import augment_cases as ac  # noqa: E402


def call_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--crop", type=int, default=368)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-samples", type=int, default=4)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "augment_bench.json"))
    a = ap.parse_args()
    N, S = a.batch, a.crop
    pad = (128, 128, 128)
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=pad), T.CropPad(pad=pad, crop_x=S, crop_y=S), T.Flip()]
    provided = np.linspace(0.1, 1.0, N)
    host = [ac.synthetic_sample(n, 480, 640, others=n % 3, scale_provided=float(provided[n])) for n in range(N)]
    resident = [dict(s, image=torch.from_numpy(s["image"]).cuda(0), mask=torch.from_numpy(s["mask"]).cuda(0)) for s in host]
    out = {"workload": "batch %d, 480x640 sources, crop %dx%d, scale_provided 0.1..1.0" % (N, S, S), "iters": a.iters}

    sd = synth.make_state_dict(1, seed=1)
    net = PoseEstimationWithMobileNet(num_refinement_stages=1)
    load_state(net, {"state_dict": sd})
    net.eval().cuda(0)
    eng = net.engine

    t0 = time.perf_counter()
    plan_host = T.plan_batch(host, transforms, random.Random(0))
    out["plan_batch_host_ms"] = (time.perf_counter() - t0) * 1e3
    plan_dev = T.plan_batch(resident, transforms, random.Random(0))
    out["resize_factor_min_max"] = [min(r["scale"] for r in plan_dev.records), max(r["scale"] for r in plan_dev.records)]
    eng.augment_batch(plan_dev, time_iters=2)
    out["kernel_ms"] = eng.augment_batch(plan_dev, time_iters=a.iters) / a.iters
    out["call_ms_device_sources"] = call_ms(lambda: eng.augment_batch(plan_dev), a.iters)
    out["call_ms_host_sources"] = call_ms(lambda: eng.augment_batch(plan_host), max(a.iters // 10, 2))

    picks = sorted(set(int(v) for v in np.linspace(0, N - 1, a.host_samples)))
    sub = T.BatchPlan([plan_host.records[i] for i in picks], [plan_host.images[i] for i in picks], [plan_host.masks[i] for i in picks],
                      [plan_host.labels[i] for i in picks], plan_host.crop_hw)
    t0 = time.perf_counter()
    want = T.apply_plan_host(sub, 8)
    out["staged_numpy_s_scaled"] = (time.perf_counter() - t0) * N / len(picks)
    out["staged_numpy_samples_timed"] = len(picks)
    got = eng.augment_batch(plan_host)
    out["elements_differing_from_numpy"] = int(sum(int((g[picks].cpu().numpy() != w).sum()) for g, w in zip(got[:3], want)))

    opt = optim.StageAdam(net, base_lr=4e-5)
    x = got[0]
    full = np.repeat(np.repeat(got[2].cpu().numpy(), 8, 1), 8, 2)
    out["train_step_ms"] = call_ms(lambda: val.train_step(net, opt, x, plan_host.labels, full), a.step_iters)
    aug = T.DeviceAugment(transforms, rng=random.Random(1))
    out["augmented_train_step_ms_device_sources"] = call_ms(lambda: val.augmented_train_step(net, opt, resident, aug), a.step_iters)
    out["kernel_share_of_train_step"] = out["kernel_ms"] / out["train_step_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
