"""Times the stage backward at the reference's training shape (train.py: batch 80 of 368 x 368), for 1 and 3 refinement stages:

  * the retaining forward (Engine.train_forward) against Engine.forward,
  * the backward's kernels per class (HIP events around every launch, Engine.profile_stage_backward),
  * torch-ROCm autograd over the same stages (tests/backward_cases.py's restatement in fp32 on the same GPU), as context.

    python tools/backward_bench.py [--batch 80] [--size 368] [--reps 3] [--scope stages|cpm|all] [--out profiles/train/backward_bench.json]

--scope cpm times the same with the cpm trained too (Engine.set_train_scope("cpm"): retained cpm activations, ELU and depthwise
gradient kernels, d_backbone not asked for); torch's autograd then starts at the cpm's input (tests/cpm_backward_cases.py).  Its
default output is profiles/train/backward_bench_cpm.json.  --scope all trains the backbone too (every backbone layer retained, strided /
dilated depthwise gradients, the stem's weight gradient, BatchNorm chain rule); torch's autograd then starts at the image
(tests/backbone_backward_cases.py) and the output is profiles/train/backward_bench_all.json.

Writes one JSON file; there is no parent figure for this path, so nothing is compared."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

import backward_cases as bc  # noqa: E402
import backbone_backward_cases as bb  # noqa: E402
import cpm_backward_cases as cc  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def one(nref, batch, size, reps, scope="stages"):
    eng = Engine(0, nref=nref)
    eng.set_train_scope(scope)
    sd = synth.make_state_dict(nref, seed=1)
    eng.load_state_dict(sd)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand((batch, 3, size, size), device="cuda", generator=g) - 0.5
    hs = size // 8
    km = torch.rand((batch, 19, hs, hs), device="cuda", generator=g)
    pm = torch.rand((batch, 38, hs, hs), device="cuda", generator=g) - 0.5
    mask = (torch.rand((batch, hs, hs), device="cuda", generator=g) > 0.1).float()
    res = dict(nref=nref, batch=batch, size=size, reps=reps, scope=scope)
    res["forward_ms"] = timed(lambda: eng.forward(x), reps)
    res["train_forward_ms"] = timed(lambda: eng.train_forward(x), reps)
    res["stage_backward_ms"] = timed(lambda: eng.stage_backward(km, pm, mask), reps)
    res["backward_classes"] = eng.profile_stage_backward(km, pm, mask, reps=reps)
    cpm, whole = scope != "stages", scope == "all"
    first = [i["index"] for i in eng.layers() if i["name"] == ("cpm.align" if cpm else "cpm.conv")][0] - (1 if cpm else 0)
    feat = x if whole else torch.from_numpy(eng.train_activation(first)).cuda()
    p = {k: v.cuda().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in sd.items()
         if k.startswith("initial_stage.") or k.startswith("refinement_stages.") or (cpm and k.startswith("cpm.")) or (whole and k.startswith("model."))}
    keys = bb.grad_keys(p) if whole else cc.grad_keys(p) if cpm else bc.grad_keys(p)

    def net(q, f):
        if whole:
            f = bb.backbone(q, f)
        return bc.stages(q, cc.cpm(q, f) if cpm else f, nref)

    def torch_step():
        f = feat.detach().requires_grad_(not whole)               # (no gradient at the image)
        total = bc.loss(net(p, f), km, pm, mask, batch)
        torch.autograd.grad(total, [p[k] for k in keys] + ([] if whole else [f]))
    res["torch_autograd_stages_fwd_bwd_ms"] = timed(torch_step, reps)
    res["torch_stages_fwd_ms"] = timed(lambda: net({k: v.detach() for k, v in p.items()}, feat), reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=368)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scope", choices=("stages", "cpm", "all"), default="stages")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "train", "backward_bench.json" if a.scope == "stages" else "backward_bench_%s.json" % a.scope)
    out = dict(device=torch.cuda.get_device_properties(0).gcnArchName, runs=[one(n, a.batch, a.size, a.reps, a.scope) for n in (1, 3)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
