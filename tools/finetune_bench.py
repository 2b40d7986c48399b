"""Measures the stage fine-tuning step (lwp_stage_adam_step, val.train_step):

  * the Adam kernel and the repack kernel alone at num_channels 128 with 1 and with 3 refinement stages (back-to-back launches
    between HIP events on scratch copies), with the bytes each moves and its share of the 8 TB/s HBM figure,
  * one full val.train_step at the reference's training shape (train.py: batch 80 of 368 x 368) next to the host route it
    replaces: gradients to the host, torch's CPU Adam with the same groups, lwp_load_weights of the whole network,
  * the loss over 50 steps on one batch of labelled synthetic frames (synthetic weights: the curve shows the loop closing, not a
    trained model).

    python tools/finetune_bench.py [--batch 80] [--size 368] [--iters 50] [--steps 50] [--scope stages|cpm|all] [--out profiles/train/finetune_bench.json]

--scope cpm runs every leg with the cpm trained too (optim.StageAdam(net, scope="cpm")) into profiles/train/finetune_bench_cpm.json;
the repack's byte count then leaves the cpm layers out, so no share of the HBM figure is given for it.  --scope all trains the
backbone as well (profiles/train/finetune_bench_all.json).

Writes one JSON file; the feature has no earlier form, so nothing is compared against a parent."""
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
from lwpose_amd import optim, synth, val  # noqa: E402
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet  # noqa: E402
from lwpose_amd.modules.load_state import load_state  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

import backbone_backward_cases as bb  # noqa: E402
import train_cases as tc  # noqa: E402

HBM_BYTES_PER_S = 8e12


def stage_blob_bytes(eng):
    first = [i["index"] for i in eng.layers() if i["name"] == "cpm.conv"][0]
    return sum((2 * i["ksize"] * i["ksize"] * ((i["cin"] + 31) // 32 * 32) + 1) * ((i["cout"] + 63) // 64 * 64) * 4
               for i in eng.layers() if i["index"] > first)


def check_blob_rule():
    """The byte count above against the graph's own layout: two more refinement stages grow the exported blob by what the
    rule gives for their layers, up to the 256-byte alignment gaps (at most two per layer)."""
    e1, e3 = Engine(0, nref=1), Engine(0, nref=3)
    grown = e3.weights_blob_bytes() - e1.weights_blob_bytes()
    rule = stage_blob_bytes(e3) - stage_blob_bytes(e1)
    layers = len(e3.layers()) - len(e1.layers())
    assert rule <= grown <= rule + 2 * 256 * layers, (rule, grown)
    return dict(blob_growth_bytes=grown, rule_bytes=rule)


def kernels(nref, iters, scope):
    eng = Engine(0, nref=nref)
    eng.set_train_scope(scope)
    eng.load_state_dict(synth.make_state_dict(nref, seed=1))
    spec, total = eng.grad_spec()
    g = torch.randn(total, device="cuda") * 1e-3
    eng.time_adam_step(g, 4e-5, iters=3)                      # warm-up
    adam_ms, repack_ms = eng.time_adam_step(g, 4e-5, iters=iters)
    adam_us, repack_us = adam_ms / iters * 1e3, repack_ms / iters * 1e3
    # Adam reads g, p, m, v and writes p, m, v; the repack reads the raw stage values once and writes both packed copies and
    # the bias row of every stage layer (cin padded to 32, cout to 64)
    adam_bytes = 7 * 4 * total
    blob_stage = stage_blob_bytes(eng)
    repack_bytes = 4 * total + blob_stage
    res = dict(nref=nref, num_channels=128, scope=scope, parameters=total, iters=iters,
               adam_us=adam_us, adam_bytes=adam_bytes, adam_share_of_8TBs=adam_bytes / (adam_us * 1e-6) / HBM_BYTES_PER_S, repack_us=repack_us)
    if scope == "stages":
        res.update(repack_bytes=repack_bytes, repack_share_of_8TBs=repack_bytes / (repack_us * 1e-6) / HBM_BYTES_PER_S)
    return res


def labelled(N, S, seed):
    rng = np.random.RandomState(seed)
    K = 18
    labels = tc.frames_to_labels(tc._crowd(rng, "coco", S, S, [1 + f % 4 for f in range(N)]), K)
    fr = synth.make_frames(N, S, S, seed0=seed)
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return x, labels


def make_net(nref=1):
    net = PoseEstimationWithMobileNet(num_refinement_stages=nref)
    sd = synth.make_state_dict(nref, seed=1)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    return net, sd


def full_step(batch, size, reps, scope):
    net, sd = make_net(1)
    x, labels = labelled(batch, size, 7)
    xc = torch.from_numpy(x).cuda()
    opt = optim.StageAdam(net, scope=scope)
    val.train_step(net, opt, xc, labels)                        # warm-up: buffers, tables, state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        val.train_step(net, opt, xc, labels)
    torch.cuda.synchronize()
    device_route = (time.perf_counter() - t0) / reps
    # the step alone on the device, and the host route it replaces
    eng = net.engine
    _, grads, _ = val.stage_gradients(net, xc, labels)
    flat = eng.flat_of(grads)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.adam_step(flat, opt.lr)
    torch.cuda.synchronize()
    device_step = (time.perf_counter() - t0) / reps
    spec, total = eng.grad_spec()
    params = {k: torch.nn.Parameter(sd[k].clone()) for k, _, _ in spec}
    groups = []
    for k, _, _ in spec:
        mult, wd = bb.group_of(k)
        groups.append({"params": [params[k]], "lr": opt.lr * mult, "weight_decay": opt.weight_decay if wd else 0})
    topt = torch.optim.Adam(groups, lr=opt.lr)
    host = dict(sd)

    def host_route():
        g = flat.cpu()
        for k, shape, off in spec:
            params[k].grad = g[off:off + params[k].numel()].view(shape)
        topt.step()
        host.update({k: p.detach() for k, p in params.items()})
        eng.load_state_dict(host)
        eng.synchronize()
    host_route()
    t0 = time.perf_counter()
    for _ in range(reps):
        host_route()
    host_step = (time.perf_counter() - t0) / reps
    return dict(batch=batch, size=size, reps=reps, train_step_ms=device_route * 1e3, device_step_ms=device_step * 1e3,
                host_route_step_ms=host_step * 1e3)


def loss_curve(steps, scope):
    net, _ = make_net(1)
    x, labels = labelled(4, 128, 11)
    opt = optim.StageAdam(net, base_lr=1e-3, scope=scope)
    curve = [sum(val.train_step(net, opt, x, labels)) for _ in range(steps)]
    curve.append(sum(val.stage_losses(net, x, labels)))
    return dict(frames=4, size=128, base_lr=1e-3, steps=steps, scope=scope, summed_stage_loss=curve)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--size", type=int, default=368)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scope", choices=("stages", "cpm", "all"), default="stages")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "train", "finetune_bench.json" if a.scope == "stages" else "finetune_bench_%s.json" % a.scope)
    out = dict(device=torch.cuda.get_device_properties(0).gcnArchName,
               kernels=[kernels(n, a.iters, a.scope) for n in (1, 3)],
               full_step=full_step(a.batch, a.size, a.reps, a.scope),
               blob_rule=check_blob_rule(),
               loss=loss_curve(a.steps, a.scope))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
