"""Cases of the cpm backward (train scope "cpm") and its differentiable restatement, shared by tests/test_cpm_backward_host.py,
tests/test_gpu_cpm_backward.py and the --scope cpm legs of tools/backward_bench.py and tools/finetune_bench.py.

``cpm`` restates the Cpm block (with_mobilenet.py:18-21: a = align(x); conv(a + trunk(a)), trunk = three depthwise 3x3 + ELU /
1x1 + ELU blocks, modules/conv.py:24-32 with bn=False) with torch.nn.functional from its 512-channel input on, in whatever dtype
its inputs have, and ``gradients`` composes it with ``backward_cases.stages`` and ``backward_cases.loss``.  The two ReLUs of the
block take their masks as an input like the stage ReLUs do (layers "cpm.align" and "cpm.conv"); ELU is differentiable
everywhere (alpha = 1: elu'(z) = exp(z) = elu(z) + 1 for z <= 0, continuous at 0), so it needs none.

The cases are those of backward_cases plus two whose maps are so small that every pixel has depthwise taps outside the map:
f (2 x 3 map, 32 channels: half a channel group of the depthwise weight-gradient kernel) and g (3 x 2 map, 128 channels)."""
import numpy as np
import torch
import torch.nn.functional as F

import backward_cases as bc
import optim_cases as oc

CASES = dict(bc.CASES)
CASES["f"] = dict(N=2, H=16, W=24, C=32, nref=0, skel="coco", seed=15, frames=340, people=9)
CASES["g"] = dict(N=3, H=24, W=16, C=128, nref=0, skel="guide5", seed=16, frames=350, people=10)

RELU_LAYERS = ("cpm.align", "cpm.conv")
ACT_NAMES = ["cpm.align"] + [n for j in range(3) for n in ("cpm.trunk.%d.dw" % j, "cpm.trunk.%d" % j)] + ["cpm.sum", "cpm"]


def cpm_keys(sd):
    return [k for k in sd if k.startswith("cpm.")]


def grad_keys(sd):
    """cpm.* then the stage keys, each in state-dict order: the gradient layout of train scope "cpm"."""
    return cpm_keys(sd) + bc.grad_keys(sd)


def cpm(sd, x, masks=None, taps=None, acts=None):
    """backbone_features from ``x``, the cpm's input (N, 512, h, w).  ``masks``: "cpm.align" / "cpm.conv" -> 0 / 1 tensors that
    replace the two ReLUs; ``taps``: filled with their pre-activations z; ``acts``: filled with every activation of ACT_NAMES
    (the oracle's tap names)."""
    def relu(name, z):
        if taps is not None:
            taps[name] = z
        if masks is None:
            return F.relu(z)
        return bc._MaskedReLU.apply(z, masks[name].to(z.dtype))

    def keep(name, t):
        if acts is not None:
            acts[name] = t
        return t

    a = keep("cpm.align", relu("cpm.align", F.conv2d(x, sd["cpm.align.0.weight"], sd["cpm.align.0.bias"])))
    t = a
    for j in range(3):
        t = keep("cpm.trunk.%d.dw" % j, F.elu(F.conv2d(t, sd["cpm.trunk.%d.0.weight" % j], None, 1, 1, 1, t.shape[1])))
        t = keep("cpm.trunk.%d" % j, F.elu(F.conv2d(t, sd["cpm.trunk.%d.2.weight" % j])))
    s = keep("cpm.sum", a + t)
    return keep("cpm", relu("cpm.conv", F.conv2d(s, sd["cpm.conv.0.weight"], sd["cpm.conv.0.bias"], 1, 1)))


def gradients(sd, xin, nref, keypoint_maps, paf_maps, mask, batch_size, loss_scale=1.0, masks=None, dtype=torch.float64):
    """(grads {key: tensor over grad_keys, "d_features", "d_backbone"}, taps {ReLU layer: z}, stage outputs, acts) in ``dtype``
    on the CPU, from the cpm's input ``xin``."""
    def cast(v):
        v = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v
        return v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()
    p = {k: cast(v) for k, v in sd.items() if k.startswith(("cpm.", "initial_stage.", "refinement_stages."))}
    keys = grad_keys(p)
    for k in keys:
        p[k].requires_grad_(True)
    x = cast(xin).requires_grad_(True)
    taps, acts = {}, {}
    feat = cpm(p, x, masks, taps, acts)
    outs = bc.stages(p, feat, nref, masks, taps)
    total = bc.loss(outs, cast(keypoint_maps), cast(paf_maps), cast(mask), batch_size, loss_scale)
    got = torch.autograd.grad(total, [p[k] for k in keys] + [feat, x])
    grads = dict(zip(keys + ["d_features", "d_backbone"], got))
    return grads, {k: v.detach() for k, v in taps.items()}, [o.detach() for o in outs], {k: v.detach() for k, v in acts.items()}


def stage_masks(layers, acts):
    """ReLU masks of the stage layers from the retained activations (``layers``: Engine.layers(), ``acts``: layer index -> NCHW
    numpy), named as backward_cases.stages names them: a merged head layer is split, a refinement block's last conv holds
    relu(z) + initial_features."""
    masks = {}
    by_name = dict((i["name"], i["index"]) for i in layers)
    for info in layers:
        nm, a = info["name"], acts.get(info["index"])
        if a is None or not nm.startswith(("initial_stage.", "refinement_stages.")) or nm.endswith(".1") and not nm.endswith(".trunk.1"):
            continue
        a = torch.from_numpy(a)
        if nm.endswith(".heads.0"):
            half = a.shape[1] // 2
            masks[nm[:-len("heads.0")] + "heatmaps.0"] = a[:, :half] > 0
            masks[nm[:-len("heads.0")] + "pafs.0"] = a[:, half:] > 0
        elif nm.startswith("refinement_stages.") and nm.endswith(".trunk.1"):
            masks[nm] = a > torch.from_numpy(acts[by_name[nm[:-len(".trunk.1")] + ".initial"]])
        else:
            masks[nm] = a > 0
    return masks


# train.py:46-48 with get_parameters.py for the cpm; the stage groups are optim_cases.group_of's
def group_of(key):
    """(learning-rate multiplier, weight decay on) of a cpm or stage parameter."""
    if not key.startswith("cpm."):
        return oc.group_of(key)
    if key.endswith(".bias"):
        return (2, False)
    parts = key.split(".")
    if parts[1] == "trunk" and parts[3] == "0":          # cpm.trunk.j.0.weight: depthwise (groups == channels)
        return (1, False)
    return (1, True)


def flat_groups(spec, base_lr):
    """Per-element (learning rate, weight-decay flag) arrays over a flat gradient-spec layout that may hold cpm keys."""
    total = sum(int(np.prod(s)) for _, s, _ in spec)
    lr = np.zeros(total, np.float64)
    decay = np.zeros(total, bool)
    for k, shape, off in spec:
        mult, wd = group_of(k)
        n = int(np.prod(shape))
        lr[off:off + n] = base_lr * mult
        decay[off:off + n] = wd
    return lr, decay


# NumPy loop statements of the two depthwise gradient formulas the kernels mirror (stride 1, dilation 1, pad 1; tap = 3 ky + kx,
# off(tap) = (ky - 1, kx - 1)); x, dz: (N, C, H, W), w: (C, 1, 3, 3)
def dw_dgrad_loops(dz, w):
    N, C, H, W = dz.shape
    dx = np.zeros_like(dz)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = y + 1 - ky, x + 1 - kx
                        if 0 <= sy < H and 0 <= sx < W:
                            dx[n, :, y, x] += dz[n, :, sy, sx] * w[:, 0, ky, kx]
    return dx


def dw_wgrad_loops(dz, x):
    N, C, H, W = dz.shape
    dw = np.zeros((C, 1, 3, 3), dz.dtype)
    for n in range(N):
        for y in range(H):
            for xx in range(W):
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = y + ky - 1, xx + kx - 1
                        if 0 <= sy < H and 0 <= sx < W:
                            dw[:, 0, ky, kx] += dz[n, :, y, xx] * x[n, :, sy, sx]
    return dw
