"""Cases of the backbone backward (train scope "all") and its differentiable restatement, shared by
tests/test_backbone_backward_host.py, tests/test_gpu_backbone_backward.py and the --scope all legs of tools/backward_bench.py and
tools/finetune_bench.py.

``backbone`` restates ``model.*`` (with_mobilenet.py:92-105: the stem conv 3 -> 32 stride 2, then eleven conv_dw blocks, depthwise
3x3 with stride 1 | 2 and dilation 1 | 2 + BatchNorm + ReLU, 1x1 + BatchNorm + ReLU; modules/conv.py:4-22) with torch.nn.functional
from the image on, BatchNorm at its running statistics (``F.batch_norm(training=False)``), in whatever dtype its inputs have.
Its 23 ReLUs take their masks as an input like the stage ReLUs do (layers "model.0", "model.i.dw", "model.i": the oracle's tap
names).  ``gradients`` composes it with ``cpm_backward_cases.cpm``, ``backward_cases.stages`` and ``backward_cases.loss``.

The cases are the smallest shapes at which the new kernels can go wrong: odd maps in front of the stride-2 layers (s, t), a
final map so small that every non-centre tap of the dilation-2 layer falls outside it (u), the 128-channel merged heads behind
the backbone (v), and several pixel ranges and workgroups per layer (w).  Frame sizes need not be multiples of 8: a map is
(H - 1) // 2 + 1 of the one before it."""
import numpy as np
import torch
import torch.nn.functional as F

import backward_cases as bc
import cpm_backward_cases as cc

BACKBONE = [(1, 1), (2, 1), (1, 1), (2, 1), (1, 1), (1, 1), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1)]   # (stride, dilation) of model.1 .. model.11

CASES = {
    "s": dict(N=2, H=36, W=44, C=32, nref=0, skel="coco", seed=21, frames=400, people=11),      # maps 18x22 -> 9x11 -> 5x6
    "t": dict(N=1, H=30, W=20, C=32, nref=0, skel="coco", seed=22, frames=410, people=12),      # maps 15x10 -> 8x5 -> 4x3
    "u": dict(N=2, H=16, W=24, C=32, nref=0, skel="coco", seed=23, frames=420, people=13),      # final map 2x3
    "v": dict(N=1, H=64, W=64, C=128, nref=1, skel="coco", seed=24, frames=430, people=14),     # the C-128 merged heads
    "w": dict(N=1, H=128, W=160, C=32, nref=0, skel="coco", seed=25, frames=440, people=15),    # several ranges / workgroups per layer
}

RELU_LAYERS = ["model.0"] + [n for i in range(1, 12) for n in ("model.%d.dw" % i, "model.%d" % i)]


def map_dims(case, level=3):
    h, w = case["H"], case["W"]
    for _ in range(level):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


def loss_mask(case):
    """backward_cases.loss_mask on the network's own map size (the frame need not be a multiple of 8)."""
    h, w = map_dims(case)
    m = np.ones((case["N"], h, w), np.float32)
    m[:, : max(1, h // 3), : max(1, w // 2)] = 0.0
    m[:, h // 2, :] = np.linspace(0.125, 0.875, w, dtype=np.float32)
    return m


def backbone_keys(sd):
    return [k for k in sd if k.startswith("model.") and "running_" not in k and "num_batches_tracked" not in k]


def grad_keys(sd):
    """model.* then cpm.* then the stage keys, each in state-dict order: the gradient layout of train scope "all"."""
    return backbone_keys(sd) + cc.grad_keys(sd)


def backbone(sd, x, masks=None, taps=None, acts=None):
    """The cpm's input (N, 512, h, w) from the image ``x`` (N, 3, H, W).  ``masks``: RELU_LAYERS name -> 0 / 1 tensor that replaces
    that ReLU; ``taps``: filled with the pre-activations z; ``acts``: filled with every activation, by the oracle's tap names."""
    def relu(name, z):
        if taps is not None:
            taps[name] = z
        y = F.relu(z) if masks is None else bc._MaskedReLU.apply(z, masks[name].to(z.dtype))
        if acts is not None:
            acts[name] = y
        return y

    def bn(t, p):
        return F.batch_norm(t, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    t = relu("model.0", bn(F.conv2d(x, sd["model.0.0.weight"], None, 2, 1), "model.0.1"))
    for i, (s, d) in enumerate(BACKBONE, start=1):
        t = relu("model.%d.dw" % i, bn(F.conv2d(t, sd["model.%d.0.weight" % i], None, s, d, d, t.shape[1]), "model.%d.1" % i))
        t = relu("model.%d" % i, bn(F.conv2d(t, sd["model.%d.3.weight" % i]), "model.%d.4" % i))
    return t


def gradients(sd, image, nref, keypoint_maps, paf_maps, mask, batch_size, loss_scale=1.0, masks=None, dtype=torch.float64):
    """(grads {key: tensor over grad_keys, "d_features", "d_backbone"}, taps {ReLU layer: z}, stage outputs, acts) in ``dtype``
    on the CPU, from the image."""
    def cast(v):
        v = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v
        return v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()
    p = {k: cast(v) for k, v in sd.items()}
    keys = grad_keys(p)
    for k in keys:
        p[k].requires_grad_(True)
    taps, acts = {}, {}
    xin = backbone(p, cast(image), masks, taps, acts)
    feat = cc.cpm(p, xin, masks, taps, acts)
    outs = bc.stages(p, feat, nref, masks, taps)
    total = bc.loss(outs, cast(keypoint_maps), cast(paf_maps), cast(mask), batch_size, loss_scale)
    got = torch.autograd.grad(total, [p[k] for k in keys] + [feat, xin])
    grads = dict(zip(keys + ["d_features", "d_backbone"], got))
    return grads, {k: v.detach() for k, v in taps.items()}, [o.detach() for o in outs], {k: v.detach() for k, v in acts.items()}


# train.py:42-45 with get_parameters.py for the backbone; the cpm and stage groups are cpm_backward_cases.group_of's
def group_of(key):
    """(learning-rate multiplier, weight decay on) of any parameter of the network."""
    if not key.startswith("model."):
        return cc.group_of(key)
    parts = key.split(".")                 # model.<i>.<j>.<weight|bias>
    i, j = int(parts[1]), int(parts[2])
    conv = (i == 0 and j == 0) or (i > 0 and j in (0, 3))
    if not conv:                           # BatchNorm: weight x1, bias x2, no weight decay
        return (2, False) if parts[3] == "bias" else (1, False)
    return (1, False) if (i > 0 and j == 0) else (1, True)      # depthwise (groups == channels) | stem, pointwise


def flat_groups(spec, base_lr):
    """Per-element (learning rate, weight-decay flag) arrays over a flat gradient-spec layout of any scope."""
    total = sum(int(np.prod(s)) for _, s, _ in spec)
    lr = np.zeros(total, np.float64)
    decay = np.zeros(total, bool)
    for k, shape, off in spec:
        mult, wd = group_of(k)
        n = int(np.prod(shape))
        lr[off:off + n] = base_lr * mult
        decay[off:off + n] = wd
    return lr, decay


# NumPy loop statements of the formulas the kernels mirror.  Depthwise 3x3 with stride s, dilation d, padding d (tap = 3 ky + kx):
# x (N, C, H, W), dz (N, C, Ho, Wo) with Ho = (H - 1) // s + 1, w (C, 1, 3, 3).
def dw_sd_dgrad_loops(dz, w, H, W, s, d):
    N, C, Ho, Wo = dz.shape
    dx = np.zeros((N, C, H, W), dz.dtype)
    for n in range(N):
        for y in range(H):
            for x in range(W):
                for ky in range(3):
                    for kx in range(3):
                        ny, nx = y + d - d * ky, x + d - d * kx
                        if ny < 0 or nx < 0 or ny % s or nx % s or ny // s >= Ho or nx // s >= Wo:
                            continue
                        dx[n, :, y, x] += dz[n, :, ny // s, nx // s] * w[:, 0, ky, kx]
    return dx


def dw_sd_wgrad_loops(dz, x, s, d):
    """(dW (C, 1, 3, 3), g (C,)): the weight gradient and the per-channel sum of dz (the folded bias gradient)."""
    N, C, Ho, Wo = dz.shape
    H, W = x.shape[2:]
    dw = np.zeros((C, 1, 3, 3), dz.dtype)
    g = np.zeros(C, dz.dtype)
    for n in range(N):
        for y in range(Ho):
            for xx in range(Wo):
                g += dz[n, :, y, xx]
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = s * y + d * (ky - 1), s * xx + d * (kx - 1)
                        if 0 <= sy < H and 0 <= sx < W:
                            dw[:, 0, ky, kx] += dz[n, :, y, xx] * x[n, :, sy, sx]
    return dw, g


def stem_wgrad_loops(dz, x):
    """(dW (32, 3, 3, 3), g (32,)) of the stem (stride 2, pad 1): dz (N, 32, Ho, Wo), x (N, 3, H, W)."""
    N, O, Ho, Wo = dz.shape
    H, W = x.shape[2:]
    dw = np.zeros((O, 3, 3, 3), dz.dtype)
    g = np.zeros(O, dz.dtype)
    for n in range(N):
        for y in range(Ho):
            for xx in range(Wo):
                g += dz[n, :, y, xx]
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = 2 * y + ky - 1, 2 * xx + kx - 1
                        if 0 <= sy < H and 0 <= sx < W:
                            dw[:, :, ky, kx] += dz[n, :, y, xx][:, None] * x[n, :, sy, sx][None, :]
    return dw, g
