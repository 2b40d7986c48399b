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

--precision bf16|fp16 [--grad-scale S] compares the backward's 16-bit mode (Engine.set_backward_precision) with fp32 mode instead:
one engine, one process, alternating windows of --reps backwards each (fp32, 16-bit, fp32, ...), the median over --windows per
mode of the per-class times, of the whole backward and of a step (train_forward + stage_backward + adam_step); the number of
non-finite elements of the 16-bit gradient; and, from one torch-ROCm fp32 autograd pass over the same restatement, the share of
the non-zero dZ elements of the dense convs that round to zero in the format at the scale.  Output:
profiles/train/backward_bench_h16.json (nref 1 only).

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
import backward_h16_cases as hc  # noqa: E402
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


def h16_compare(nref, batch, size, reps, scope, precision, scale, windows):
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
    res = dict(nref=nref, batch=batch, size=size, reps=reps, windows=windows, scope=scope, precision=precision, grad_scale=scale)
    eng.train_forward(x)
    modes = (("fp32", 1.0), (precision, scale))
    # the gradient and the dZ statistics first: the timed steps below move the weights
    eng.set_backward_precision(precision, scale)
    flat = eng.flat_of(eng.stage_backward(km, pm, mask)[0])
    res["gradient_elements"] = int(flat.numel())
    res["nonfinite_gradient_elements"] = int((~torch.isfinite(flat)).sum())
    cpm, whole = scope != "stages", scope == "all"
    first = [i["index"] for i in eng.layers() if i["name"] == ("cpm.align" if cpm else "cpm.conv")][0] - (1 if cpm else 0)
    feat = x if whole else torch.from_numpy(eng.train_activation(first)).cuda()
    p = {k: v.cuda().requires_grad_(v.is_floating_point() and "running_" not in k) for k, v in sd.items()}
    keys = bb.grad_keys(p) if whole else cc.grad_keys(p) if cpm else bc.grad_keys(p)
    sim = hc.Sim("fp32", scale, count_as=precision)
    with hc.installed(sim):
        f = feat.detach().requires_grad_(not whole)
        if whole:
            f = bb.backbone(p, f)
        total = bc.loss(bc.stages(p, cc.cpm(p, f) if cpm else f, nref), km, pm, mask, batch)
        torch.autograd.grad(total, [p[k] for k in keys])
    res["dz_max"] = sim.stats["max_dz"]
    res["dz_nonzero"] = sim.stats["nonzero"]
    res["dz_rounded_to_zero_share"] = sim.stats["flushed"] / max(1, sim.stats["nonzero"])
    del p, f, total

    def step():
        eng.train_forward(x)
        eng.adam_step(eng.flat_of(eng.stage_backward(km, pm, mask)[0]), 4e-5, (0.9, 0.999), 1e-8, 5e-4)
    names = ("elementwise", "dgrad", "wgrad", "reduce")
    samples = dict((m[0], dict(backward=[], step=[], classes=dict((n, []) for n in names))) for m in modes)
    for _ in range(windows):
        for name, sc in modes:
            eng.set_backward_precision(name, sc)
            eng.train_forward(x)
            samples[name]["backward"].append(timed(lambda: eng.stage_backward(km, pm, mask), reps))
            cls = eng.profile_stage_backward(km, pm, mask, reps=reps)
            for n in names:
                samples[name]["classes"][n].append(cls[n]["ms"])
            samples[name]["step"].append(timed(step, reps))
    med = lambda v: float(np.median(v))
    for name, _ in modes:
        sm = samples[name]
        res[name] = dict(stage_backward_ms=med(sm["backward"]), step_ms=med(sm["step"]), backward_classes_ms=dict((n, med(sm["classes"][n])) for n in names),
                         stage_backward_ms_windows=sm["backward"])
    eng.set_backward_precision("fp32", 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=368)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scope", choices=("stages", "cpm", "all"), default="stages")
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", choices=("fp32", "bf16", "fp16"), default="fp32")
    ap.add_argument("--grad-scale", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if a.precision != "fp32":
        a.out = a.out or os.path.join(ROOT, "profiles", "train", "backward_bench_h16.json")
        out = dict(device=torch.cuda.get_device_properties(0).gcnArchName,
                   runs=[h16_compare(1, a.batch, a.size, a.reps, a.scope, a.precision, a.grad_scale, a.windows)])
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "train", "backward_bench.json" if a.scope == "stages" else "backward_bench_%s.json" % a.scope)
    out = dict(device=torch.cuda.get_device_properties(0).gcnArchName, runs=[one(n, a.batch, a.size, a.reps, a.scope) for n in (1, 3)])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
