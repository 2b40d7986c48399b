"""Statements, shapes and the end-to-end restatement for the backward's 16-bit mode (lwp_set_backward_precision: bf16 / fp16
operands of the two MFMA products of the dense-conv gradients), shared by tests/test_backward_h16_host.py,
tests/test_gpu_backward_h16.py and tools/backward_bench.py.  No GPU in here.

Kernels alone: ``dense_results_h16`` is ``backward_kernel_cases.dense_results`` on the operands as the kernels see them: dz
multiplied by the power of two S = grad_scale, rounded once to the format and divided by S again (the kernels multiply the f32
accumulator by 1 / S: exact), x and w rounded once; db from the unrounded dz.  Everything in float64.

End to end: ``sim_gradients`` runs the float64 restatements of backward_cases / cpm_backward_cases / backbone_backward_cases with
every dense stride-1 conv (and the BatchNorm behind it, if any) replaced by an autograd Function whose backward rounds where the
kernels round: dZ S, the layer's input x, and the folded weight as float32 (s W for a conv with BatchNorm behind it, s = gamma /
sqrt(var + 1e-5): what the forward blob and pw_fold hold).  The depthwise convs, the stem, BatchNorm's chain rule, the
activations and the loss stay float64, as they stay f32 on the device."""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import backbone_backward_cases as bb
import backward_cases as bc
import backward_kernel_cases as kc
import cpm_backward_cases as cc
from exact_cases import ROUND

U2 = 2.0 ** -23
# (precision, grad_scale) of the integer fixtures; the normal fixtures run the same three
MODES = (("bf16", 1.0), ("fp16", 1.0), ("fp16", 64.0))
# (N, H, W, cout, cin, ks, dil, pad mode): backward_kernel_cases' shapes and the smallest ones that cross the 32-deep K step
K_STEP_SHAPES = [
    (1, 3, 11, 33, 40, 1, 1, "graph"),      # M = 33 and cout = 33: one past a K step of wgrad and of dgrad
    (1, 1, 31, 31, 8, 3, 1, "graph"),       # M = 31 and cout = 31: one short of a K step; a one-row map under a 3x3
    (2, 4, 4, 64, 16, 1, 1, "raw"),         # M = 32 and cout = 64: exactly one and two K steps, raw padding
]
DENSE_SHAPES = kc.DENSE_SHAPES + K_STEP_SHAPES
CHUNKS = (0, 16, 48)                        # max_chunk: the plan's own ranges, half a K step, one and a half


def round16(a, precision, rounding=ROUND):
    """A NumPy array rounded to ``precision`` (through float32, as the kernels' operands are), as float64."""
    return rounding[precision](torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def dense_results_h16(dz, x, w, dil, dx0, dw0, db0, acc_from, no_bias, accumulate, precision, grad_scale, rounding=ROUND, unscale=True,
                      round_db=False):
    """(results, sum|terms|) as ``kc.dense_results`` gives them, in float64, for the 16-bit kernels.  The last three arguments are
    the mutants of tests/test_backward_h16_host.py: another rounding, a missing 1 / grad_scale, db summed over the rounded dz."""
    S = float(grad_scale)
    f = lambda a: np.asarray(a, np.float64)
    dzr = round16(f(dz) * S, precision, rounding)
    if unscale:
        dzr = dzr / S
    res, terms = kc.dense_results(dzr, round16(x, precision, rounding), round16(w, precision, rounding), dil, f(dx0), f(dw0), f(db0), acc_from,
                                  no_bias, accumulate)
    if not no_bias and not round_db:
        db, db_abs = kc.dense_bias(f(dz)), kc.dense_bias(f(dz), abs=True)
        if accumulate:
            db, db_abs = f(db0) + db, np.abs(f(db0)) + db_abs
        res["db"], terms["db"] = db, db_abs
    return res, terms


def bound_ratios_h16(got, want, terms, depths):
    """``kc.bound_ratios`` at (depth + 8) 2^-23 sum|terms|: twice the f32 kernels' constant, see tests/test_gpu_backward_h16.py."""
    r = kc.bound_ratios(got, want, terms, depths)
    return dict((k, v / 2) for k, v in r.items())


# ---------------------------------------------------------------------------------------------- end to end
class _H16Conv(torch.autograd.Function):
    """conv2d(x, w, b, 1, pad, dil) whose backward is the 16-bit kernels': operands rounded, products and sums exact (float64)."""
    @staticmethod
    def forward(ctx, x, w, b, pad, dil, sim):
        ctx.save_for_backward(x, w)
        ctx.conf = (pad, dil, sim, b is not None)
        return F.conv2d(x, w, b, 1, pad, dil)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        pad, dil, sim, has_b = ctx.conf
        gs = sim.scaled(g)
        dx = torch.nn.grad.conv2d_input(x.shape, sim.rnd(w), gs, 1, pad, dil) if ctx.needs_input_grad[0] else None
        dw = torch.nn.grad.conv2d_weight(sim.rnd(x), w.shape, gs, 1, pad, dil)
        return dx, dw, (g.sum((0, 2, 3)) if has_b else None), None, None, None


class _H16ConvBN(torch.autograd.Function):
    """batch_norm(conv2d(x, W, b, 1, pad, dil)) at running statistics.  The kernels differentiate the folded conv: g is dZ, the
    data gradient reads float32(s W), the weight gradient gives G and the column sums g_b, bn_chain turns them into the raw
    parameters' gradients (backward_cases.bn_chain)."""
    @staticmethod
    def forward(ctx, x, W, b, mean, var, gamma, beta, pad, dil, sim):
        ctx.save_for_backward(x, W, mean, var, gamma)
        ctx.b = b
        ctx.conf = (pad, dil, sim)
        return F.batch_norm(F.conv2d(x, W, b, 1, pad, dil), mean, var, gamma, beta, False, 0.0, 1e-5)

    @staticmethod
    def backward(ctx, g):
        x, W, mean, var, gamma = ctx.saved_tensors
        pad, dil, sim = ctx.conf
        b = ctx.b
        inv = 1.0 / torch.sqrt(var + 1e-5)
        s = gamma * inv
        folded = sim.fold(W * s.view(-1, 1, 1, 1))
        gs = sim.scaled(g)
        dx = torch.nn.grad.conv2d_input(x.shape, sim.rnd(folded), gs, 1, pad, dil) if ctx.needs_input_grad[0] else None
        G = torch.nn.grad.conv2d_weight(sim.rnd(x), W.shape, gs, 1, pad, dil)
        gb = g.sum((0, 2, 3))
        shift = (b.detach() - mean) if b is not None else -mean
        dgamma = ((W * G).sum((1, 2, 3)) + gb * shift) * inv
        return dx, s.view(-1, 1, 1, 1) * G, (s * gb if b is not None else None), None, None, dgamma, gb, None, None, None


class Sim(object):
    """Stands in for torch.nn.functional inside the restatement modules.  ``stats``: the largest |dZ| any dense conv saw, the
    number of non-zero dZ elements and how many of them became zero at the scale, in ``count_as`` where that is another format
    than the one the backward rounds to (tools/backward_bench.py counts on an unrounded fp32 pass)."""
    def __init__(self, precision, grad_scale, count_as=None):
        self.round, self.S = ROUND[precision], float(grad_scale)
        self.count = ROUND[count_as or precision]
        # the folded weight exists as float32 on the device (left alone with "fp32": that mode is the float64 restatement itself)
        self.fold = (lambda t: t) if precision == "fp32" else (lambda t: t.to(torch.float32).to(torch.float64))
        self.pending = {}
        self.stats = dict(max_dz=0.0, nonzero=0, flushed=0)

    def __getattr__(self, name):
        return getattr(F, name)

    def rnd(self, t):
        return self.round(t.detach())

    def scaled(self, g):
        gs = self.round(g * self.S) / self.S
        nz = g != 0
        self.stats["max_dz"] = max(self.stats["max_dz"], float(g.abs().max()))
        self.stats["nonzero"] += int(nz.sum())
        self.stats["flushed"] += int((nz & ((gs if self.count is self.round else self.count(g * self.S)) == 0)).sum())
        return gs

    def conv2d(self, x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if groups != 1 or stride != 1:                     # depthwise convs and the stem stay as they are
            return F.conv2d(x, w, b, stride, padding, dilation, groups)
        y = _H16Conv.apply(x, w, b, padding, dilation, self)
        self.pending = {id(y): (y, x, w, b, padding, dilation)}
        return y

    def batch_norm(self, t, mean, var, gamma, beta, training, momentum, eps):
        p = self.pending.pop(id(t), None)
        if p is None:
            return F.batch_norm(t, mean, var, gamma, beta, training, momentum, eps)
        _, x, w, b, padding, dilation = p
        return _H16ConvBN.apply(x, w, b, mean, var, gamma, beta, padding, dilation, self)


@contextlib.contextmanager
def installed(sim):
    mods = (bc, cc, bb)
    saved = [m.F for m in mods]
    for m in mods:
        m.F = sim
    try:
        yield
    finally:
        for m, f in zip(mods, saved):
            m.F = f


GRADIENTS = {"stages": bc.gradients, "cpm": cc.gradients, "all": bb.gradients}


def sim_gradients(scope, precision, grad_scale, *args, **kwargs):
    """(grads as ``GRADIENTS[scope](*args, **kwargs)`` returns them first, stats) with the dense convs' backward in ``precision``
    ("fp32": no rounding, which must reproduce the plain restatement)."""
    sim = Sim(precision, grad_scale)
    with installed(sim):
        out = GRADIENTS[scope](*args, **kwargs)
    return out[0], sim.stats


def fp16_scale(max_dz):
    """The largest power of two S in [1, 2^24] with max|dz| S < 2^15."""
    e = math.frexp(max_dz)[1]               # max_dz < 2^e
    return float(2.0 ** min(24, max(0, 15 - e)))


def _smallest(cases):
    return min(sorted(cases), key=lambda k: cases[k]["N"] * cases[k]["H"] * cases[k]["W"])


# scope -> (case table, the name of its smallest case by pixels of the frames)
E2E_CASES = dict((scope, (cases, _smallest(cases))) for scope, cases in (("stages", bc.CASES), ("cpm", cc.CASES), ("all", bb.CASES)))
