"""Cases of the stage backward and its differentiable float64 restatement, shared by tests/test_backward_host.py,
tests/test_gpu_backward.py and tools/backward_bench.py.

``stages`` restates initial_stage / refinement_stages (with_mobilenet.py:25-86) with torch.nn.functional from the cpm output on,
BatchNorm at running statistics (``F.batch_norm(training=False)``), in whatever dtype its inputs have; ``loss`` is
train.py:99-102 with modules/loss.py's formula.  Gradients come from torch.autograd.

Branch taken: a gradient is discontinuous across a ReLU kink, and an fp32 and a float64 forward disagree on the sign of a
pre-activation within rounding of zero, so ``stages`` can take its ReLU masks as an input (forward z * mask, backward g * mask)
and the reference differentiates the branch the device took.  ``mask_deviation`` measures how far the given masks are from
the float64 forward's own z > 0, so that this cannot hide a kernel fault: at most 1e-4 of a layer's elements may differ and
each of them must have |z64| <= 1e-4 max|z64| of its layer.  The case seeds below were chosen with torch's fp32 CPU forward as
the stand-in for the device (tests/test_backward_host.py holds the small cases to it); only the seeds are kept."""
import numpy as np
import torch
import torch.nn.functional as F

import train_cases as tc

# name: frames, H, W, num_channels, nref, skeleton, weight seed, frame seed, persons seed
CASES = {
    "a": dict(N=2, H=64, W=64, C=32, nref=1, skel="coco", seed=11, frames=300, people=5),
    "b": dict(N=3, H=40, W=56, C=32, nref=2, skel="guide5", seed=12, frames=310, people=6),
    "c": dict(N=1, H=368, W=368, C=128, nref=1, skel="coco", seed=13, frames=320, people=7),
    "d": dict(N=1, H=32, W=40, C=32, nref=0, skel="coco", seed=14, frames=330, people=8),
    # 8 refinement stages: 18 stage tensors, so the loss and its gradient take a second launch (16 tensors to a launch).  Its
    # layers have 1920 elements or fewer, so MASK_FRACTION allows not one element off the float64 branch.  Of the two weight
    # seeds tried on the CPU (31, 32: no deviation with either), 32 keeps every pre-activation further from zero: the
    # smallest |z64| / max|z64| of any layer is 4.4e-7 against 4.0e-8, which is below float32's resolution.
    "n8": dict(N=2, H=40, W=48, C=32, nref=8, skel="guide5", seed=32, frames=500, people=21),
}
MASK_FRACTION = 1e-4      # of a layer's elements may take another branch than the float64 forward ...
MASK_MARGIN = 1e-4        # ... each within this fraction of the layer's max |z64| of zero


def channels(case):
    K, lk, _ = tc.skeleton(case["skel"])
    return K + 1, 2 * len(lk)


def persons(case):
    """(kpts (N, Pmax, K, 3), n_persons) in the frame's pixel coordinates."""
    rng = np.random.RandomState(case["people"])
    K = tc.skeleton(case["skel"])[0]
    frames = [[tc._person(rng, case["skel"], case["H"], case["W"]) for _ in range(1 + f % 2)] for f in range(case["N"])]
    return tc.frames_to_arrays(frames, K)


def loss_mask(case):
    """(N, h, w) float32: ones, a block of zeros and a band of fractional values."""
    h, w = case["H"] // 8, case["W"] // 8
    m = np.ones((case["N"], h, w), np.float32)
    m[:, : max(1, h // 3), : max(1, w // 2)] = 0.0
    m[:, h // 2, :] = np.linspace(0.125, 0.875, w, dtype=np.float32)
    return m


class _MaskedReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, mask):
        ctx.save_for_backward(mask)
        return z * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * mask, None


def stages(sd, feat, nref, masks=None, taps=None):
    """Stage outputs [heat0, paf0, heat1, ...] from ``feat`` (the cpm output).  ``masks``: layer name -> 0 / 1 tensor that
    replaces that layer's ReLU; ``taps``: filled with every ReLU layer's pre-activation z."""
    def relu(name, z):
        if taps is not None:
            taps[name] = z
        if masks is None:
            return F.relu(z)
        return _MaskedReLU.apply(z, masks[name].to(z.dtype))

    def conv(x, p, pad=0, dil=1):
        return F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], 1, pad, dil)

    def bn(x, p):
        return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, 1e-5)

    def heads(t, p):
        hh = relu(p + ".heatmaps.0", conv(t, p + ".heatmaps.0.0"))
        qh = relu(p + ".pafs.0", conv(t, p + ".pafs.0.0"))
        return [conv(hh, p + ".heatmaps.1.0"), conv(qh, p + ".pafs.1.0")]

    t = feat
    for j in range(3):
        t = relu("initial_stage.trunk.%d" % j, conv(t, "initial_stage.trunk.%d.0" % j, 1, 1))
    outs = heads(t, "initial_stage")
    for k in range(nref):
        p = "refinement_stages.%d" % k
        t = torch.cat([feat, outs[-2], outs[-1]], 1)
        for b in range(5):
            q = "%s.trunk.%d" % (p, b)
            ini = relu(q + ".initial", conv(t, q + ".initial.0"))
            u = relu(q + ".trunk.0", bn(conv(ini, q + ".trunk.0.0", 1, 1), q + ".trunk.0.1"))
            u = relu(q + ".trunk.1", bn(conv(u, q + ".trunk.1.0", 2, 2), q + ".trunk.1.1"))
            t = ini + u
        outs.extend(heads(t, p))
    return outs


def loss(outs, keypoint_maps, paf_maps, mask, batch_size, loss_scale=1.0):
    """train.py:99-102: loss_scale * sum_i sum(((out_i - target_i) * mask)^2) / 2 / batch_size."""
    total = 0.0
    for i, o in enumerate(outs):
        t = paf_maps if i % 2 else keypoint_maps
        total = total + (((o - t) * mask[:, None]) ** 2).sum() / 2 / batch_size
    return total * loss_scale


def grad_keys(sd):
    return [k for k in sd if (k.startswith("initial_stage.") or k.startswith("refinement_stages."))
            and "running_" not in k and "num_batches_tracked" not in k]


def gradients(sd, feat, nref, keypoint_maps, paf_maps, mask, batch_size, loss_scale=1.0, masks=None, dtype=torch.float64):
    """(grads {key: tensor, "d_features": tensor}, taps {layer: z}) in ``dtype`` on the CPU."""
    def cast(v):
        v = torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v
        return v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()
    p = {k: cast(v) for k, v in sd.items() if k.startswith("initial_stage.") or k.startswith("refinement_stages.")}
    keys = grad_keys(p)
    for k in keys:
        p[k].requires_grad_(True)
    f = cast(feat).requires_grad_(True)
    taps = {}
    outs = stages(p, f, nref, masks, taps)
    total = loss(outs, cast(keypoint_maps), cast(paf_maps), cast(mask), batch_size, loss_scale)
    got = torch.autograd.grad(total, [p[k] for k in keys] + [f])
    grads = dict(zip(keys + ["d_features"], got))
    return grads, {k: v.detach() for k, v in taps.items()}, [o.detach() for o in outs]


def own_masks(taps):
    return {k: (z > 0) for k, z in taps.items()}


def mask_deviation(masks, taps64):
    """Per layer (fraction of elements whose mask differs from z64 > 0, largest |z64| / max|z64| among them)."""
    out = {}
    for k, z in taps64.items():
        diff = masks[k].bool() != (z > 0)
        n = int(diff.sum())
        out[k] = (n / diff.numel(), float(z[diff].abs().max() / z.abs().max()) if n else 0.0)
    return out


def check_mask_deviation(masks, taps64):
    for k, (frac, margin) in mask_deviation(masks, taps64).items():
        assert frac <= MASK_FRACTION and margin <= MASK_MARGIN, "layer %s: %.3g of the elements off the float64 branch, |z| up to %.3g of the layer's max" % (k, frac, margin)


def err(g, g64):
    """e(g) = max|g - g64| / max|g64|."""
    g64 = g64.double()
    return float((g.double() - g64).abs().max() / g64.abs().max())


def bn_chain(G, g, W, b, gamma, mean, var, eps=1e-5):
    """Gradients of the raw parameters of conv + BatchNorm at running statistics from the gradients G / g of the folded weight
    s W / folded bias s (b - mean) + beta, s = gamma / sqrt(var + eps): (dW, db, dgamma, dbeta).  csrc/bwd_kernels.hip's
    bn_chain_kernel is this in float64."""
    G, g, W = np.asarray(G, np.float64), np.asarray(g, np.float64), np.asarray(W, np.float64)
    inv = 1.0 / np.sqrt(np.asarray(var, np.float64) + eps)
    s = np.asarray(gamma, np.float64) * inv
    dot = (W * G).reshape(len(g), -1).sum(1)
    return s.reshape(-1, 1, 1, 1) * G, s * g, (dot + g * (np.asarray(b, np.float64) - np.asarray(mean, np.float64))) * inv, g.copy()
