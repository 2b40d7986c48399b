"""Training targets and per-stage loss: device time against the host renderings, and the first label-grounded comparison of the
three engine dtypes.

    python tools/targets_bench.py [--batch 80] [--size 368] [--iters 200] [--out profiles/train/targets_bench.json]

The reference's training shape: batch 80 of 368 x 368 frames, stride 8 (46 x 46 maps), sigma 7, PAF thickness 1, with 1, 8 and
32 persons per frame.  Records
  - kernel time of the targets (lwp_time_train_targets: HIP events around ``iters`` back-to-back launches on the engine's stream
    after one upload and a warm-up, no synchronise in between), and beside it the time of a whole Engine.train_targets call
    (upload of the person counts, launch, synchronise: what a caller waits for);
  - kernel time of the loss over 2 and 6 stage tensors (lwp_time_stage_losses, nref 0 / 2 engines: stage_loss_kernel and its
    reduce, back to back) with the bytes per second it reads against the 8 TB/s HBM figure the project uses, and the time of a
    whole Engine.stage_losses call (launches, copy-back of the sums, synchronise);
  - host time of the vectorised NumPy oracle and of the reference-style pixel loops of tests/train_cases.py (the loops on a
    slice of the batch, scaled);
  - val.stage_losses of one set of synthetic labelled frames for fp32, bf16 and fp16."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth, val  # noqa: E402
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet  # noqa: E402
from lwpose_amd.modules.load_state import load_state  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402
import train_cases as tc  # noqa: E402

HBM_BYTES_PER_S = 8e12


def call_ms(fn, iters):
    """host clock around ``iters`` whole calls, each of which ends in its own synchronise"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def kernel_ms(fn, iters):
    """fn(time_iters) -> ms of that many back-to-back launches (HIP events inside the library); warm-up first"""
    fn(2)
    return fn(iters) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=368)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--loop-frames", type=int, default=2, help="frames the pixel-loop rendering is timed on (scaled to the batch)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "targets_bench.json"))
    a = ap.parse_args()
    N, S = a.batch, a.size
    K, lk, lp = tc.skeleton("coco")
    limbs = tc.limb_rows(lk, lp)
    out = {"workload": "batch %d x %dx%d, stride 8, sigma 7, thickness 1" % (N, S, S), "iters": a.iters, "targets": {}, "loss": {}}
    eng = Engine(0)
    for persons in (1, 8, 32):
        rng = np.random.RandomState(persons)
        kpts, n = tc.frames_to_arrays(tc._crowd(rng, "coco", S, S, [persons] * N), K)
        d = torch.from_numpy(kpts).cuda(0)
        k_ms = kernel_ms(lambda it: eng.train_targets(d, n, (S, S), time_iters=it), a.iters)
        c_ms = call_ms(lambda: eng.train_targets(d, n, (S, S)), a.iters)
        t0 = time.perf_counter()
        want = tc.targets(kpts, n, S, S, 8, 7, 1, K, limbs)
        t_vec = time.perf_counter() - t0
        t0 = time.perf_counter()
        tc.targets_loops(kpts[:a.loop_frames], n[:a.loop_frames], S, S, 8, 7, 1, K, limbs)
        t_loop = (time.perf_counter() - t0) * N / a.loop_frames
        km, pm = eng.train_targets(d, n, (S, S))
        u = max(int(tc.ulp_distance(km.cpu().numpy(), want[0]).max()), int(tc.ulp_distance(pm.cpu().numpy(), want[1]).max()))
        out["targets"]["%d_persons" % persons] = {"kernel_ms": k_ms, "call_ms": c_ms, "numpy_vectorised_s": t_vec, "pixel_loops_s_scaled": t_loop,
                                                  "pixel_loops_frames_timed": a.loop_frames, "max_ulp_vs_numpy": u}
    h = S // 8
    for nref in (0, 2):
        e = Engine(0, nref=nref)
        n_t = 2 * (nref + 1)
        g = torch.Generator(device="cuda:0").manual_seed(nref)
        outs = [torch.rand((N, 38 if i % 2 else 19, h, h), device="cuda:0", generator=g) for i in range(n_t)]
        kt, pt = torch.rand((N, 19, h, h), device="cuda:0", generator=g), torch.rand((N, 38, h, h), device="cuda:0", generator=g)
        m = (torch.rand((N, h, h), device="cuda:0", generator=g) > 0.2).float()
        k_ms = kernel_ms(lambda it: e.stage_losses(outs, kt, pt, m, time_iters=it), a.iters)
        c_ms = call_ms(lambda: e.stage_losses(outs, kt, pt, m), a.iters)
        nbytes = 4 * (sum(o.numel() for o in outs) + kt.numel() + pt.numel() + m.numel())
        out["loss"]["%d_tensors" % n_t] = {"kernel_ms": k_ms, "call_ms": c_ms, "bytes_read": nbytes, "kernel_bytes_per_s": nbytes / (k_ms * 1e-3),
                                           "kernel_fraction_of_8TBps": nbytes / (k_ms * 1e-3) / HBM_BYTES_PER_S}
    # one set of synthetic labelled frames through the three stacks (synthetic weights: the figures compare the dtypes, they
    # say nothing about a trained model)
    rng = np.random.RandomState(7)
    fr = synth.make_frames(4, S, S, seed0=0)
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    labels = tc.frames_to_labels(tc._crowd(rng, "coco", S, S, [3, 1, 5, 2]), K)
    mask = (rng.rand(4, S, S) > 0.1).astype(np.float32)
    sd = synth.make_state_dict(1, seed=1)
    out["stage_losses_by_dtype"] = {}
    for dtype in ("fp32", "bf16", "fp16"):
        net = PoseEstimationWithMobileNet(num_refinement_stages=1, dtype=dtype)
        load_state(net, {"state_dict": sd})
        net.eval().cuda(0)
        out["stage_losses_by_dtype"][dtype] = val.stage_losses(net, x, labels, mask)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
