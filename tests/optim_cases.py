"""Cases of the stage fine-tuning step and its float64 restatement, shared by tests/test_optim_host.py, tests/test_gpu_optim.py and
tools/finetune_bench.py.

``adam_ref`` restates torch's single-tensor Adam (torch/optim/adam.py, no amsgrad, not maximize) in float64 NumPy, statement by
statement in the order the device kernel keeps: the kernel computes the same doubles and rounds each of its three stores to
float32 once.  ``group_of`` restates train.py:41-55 for the stage parameters.  ``float64_loop`` is the fine-tuning loop of case d
on one fixed batch; its learning rate and its loss at step 0 and step 20 are pinned below (tests/test_optim_host.py recomputes
them)."""
import numpy as np
import torch

import backward_cases as bc
import train_cases as tc

# a, b, d of backward_cases; e runs the merged head pair and the 128-wide fragment tiles of the repack
CASES = {k: bc.CASES[k] for k in ("a", "b", "d")}
CASES["e"] = dict(N=1, H=32, W=40, C=128, nref=1, skel="coco", seed=15, frames=340, people=9)

BETAS, EPS, WEIGHT_DECAY = (0.9, 0.999), 1e-8, 5e-4

# ---- the pinned float64 loop of case d: 20 steps of backward_cases.gradients + adam_ref on one fixed batch.  LOOP_LR is chosen
# (not fitted to the device) so that the loop at least halves the loss: Adam's first steps move every parameter by about
# lr * multiplier, the synthetic weights are of order 0.01 .. 0.1, so a base rate of 1e-3 changes them visibly within 20 steps.
LOOP_STEPS = 20
LOOP_LR = 1e-3
LOOP_LOSS0 = 14.816865145594782
LOOP_LOSS20 = 0.34552459633305466


# train.py:41-55 for the stage parameters: (learning-rate multiplier, weight decay on) of the six groups
GROUPS = [(1, True), (2, False), (4, True), (8, False), (1, False), (2, False)]
GROUP_NAMES = ["initial_stage conv weight", "initial_stage conv bias", "refinement_stages conv weight",
               "refinement_stages conv bias", "refinement_stages BN weight", "refinement_stages BN bias"]


def kind_of(key):
    """Index into GROUPS of a stage parameter's group."""
    refine = key.startswith("refinement_stages.")
    if not refine and not key.startswith("initial_stage."):
        raise KeyError(key)
    parts = key.split(".")
    bias = {"weight": 0, "bias": 1}[parts[-1]]
    if refine and len(parts) >= 4 and parts[-2] == "1" and parts[-4] == "trunk":     # refinement_stages.K.trunk.B.trunk.{0,1}.1.*
        return 4 + bias
    return (2 if refine else 0) + bias


def group_of(key):
    """(learning-rate multiplier, weight decay on) of a stage parameter under train.py:41-55."""
    return GROUPS[kind_of(key)]


def adam_ref(p, g, m, v, t, lr, decay, betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY):
    """One step on float64 arrays (any shape; ``lr`` and ``decay`` scalars or arrays that broadcast): returns the new
    (p, m, v) in float64, unrounded.  t is the step count AFTER the increment (1 for the first step)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = float(betas[0]), float(betas[1])
    g = np.where(decay, g + weight_decay * p, g)
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    denom = np.sqrt(v) / np.sqrt(bc2) + eps
    p = p - (lr / bc1) * m / denom
    return p, m, v


def flat_groups(spec, base_lr):
    """Per-element (learning rate, weight-decay flag) arrays over the flat gradient-spec layout."""
    total = sum(int(np.prod(s)) for _, s, _ in spec)
    lr = np.zeros(total, np.float64)
    decay = np.zeros(total, bool)
    for k, shape, off in spec:
        mult, wd = group_of(k)
        n = int(np.prod(shape))
        lr[off:off + n] = base_lr * mult
        decay[off:off + n] = wd
    return lr, decay


def crafted_gradients(spec, step, seed=0):
    """Flat float32 gradients: per parameter a cycle of zeros, +-1e-30, +-1e-8, values near 1 and +-1e4, shuffled per step;
    the whole second parameter is zero."""
    rng = np.random.RandomState(seed * 100 + step)
    total = sum(int(np.prod(s)) for _, s, _ in spec)
    flat = np.zeros(total, np.float32)
    for i, (k, shape, off) in enumerate(spec):
        n = int(np.prod(shape))
        if i == 1:
            continue
        kind = rng.randint(0, 5, n)
        sign = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
        near1 = 1.0 + (rng.rand(n) - 0.5) * 1e-3
        mag = np.choose(kind, [np.zeros(n), np.full(n, 1e-30), np.full(n, 1e-8), near1, np.full(n, 1e4)])
        flat[off:off + n] = (sign * mag).astype(np.float32)
    return flat


def ulp_distance(a, b):
    """Element-wise distance in float32 steps (NaN never occurs in the inputs the tests pass)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def case_state(name):
    c = CASES[name]
    NH, NP = bc.channels(c)
    from lwpose_amd import synth
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, NH, NP, sd, x


def float64_loop(steps=LOOP_STEPS, base_lr=LOOP_LR):
    """Case d in float64 from the oracle's cpm output: the summed loss before every step and after the last one."""
    from oracle import net_ref
    c, NH, NP, sd, x = case_state("d")
    taps = {}
    net_ref.forward64(sd, torch.from_numpy(x), c["nref"], taps, stop_after="cpm")
    feat = taps["cpm"]
    K, lk, lp = tc.skeleton(c["skel"])
    kp, n = bc.persons(c)
    km, pm = tc.targets(kp, n, c["H"], c["W"], 8, 7, 1, K, tc.limb_rows(lk, lp))
    km, pm, mask = torch.from_numpy(km), torch.from_numpy(pm), torch.from_numpy(bc.loss_mask(c))
    keys = bc.grad_keys(sd)
    p = {k: sd[k].double().numpy() for k in keys}
    m = {k: np.zeros_like(p[k]) for k in keys}
    v = {k: np.zeros_like(p[k]) for k in keys}
    losses = []

    def evaluate():
        cur = dict(sd)
        cur.update({k: torch.from_numpy(p[k]) for k in keys})
        grads, _, outs = bc.gradients(cur, feat, c["nref"], km, pm, mask, c["N"])
        losses.append(float(bc.loss(outs, km.double(), pm.double(), mask.double(), c["N"])))
        return grads
    for t in range(1, steps + 1):
        grads = evaluate()
        for k in keys:
            mult, wd = group_of(k)
            p[k], m[k], v[k] = adam_ref(p[k], grads[k].numpy(), m[k], v[k], t, base_lr * mult, wd)
    evaluate()
    return losses
