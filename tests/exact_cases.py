"""Exact-arithmetic fixtures of the conv stack: weights and frames for which every product and every partial sum of the layer
under test is exactly representable in fp32, so that no summation order, MFMA shape, split-K, tile size or fusion can change
a bit, and a float64 restatement that rounds where the 16-bit path rounds must equal the device on EVERY element.

Plain Python (numpy + torch on the CPU, no GPU); shared by tests/test_exact_host.py and tests/test_gpu_exact.py.

The condition.  A set of finite terms is order-independently exact in fp32 when every term is an integer multiple of one
power of two q and sum(|t|) < 2^24 q: every partial sum in every order is then a multiple of q below 2^24 q, hence
representable (an fmaf chain included).  ``exactness`` measures 24 - log2(max sum|t| / q) for every reduction up to the
layer under test, with q the product of the smallest set bit of the inputs and of the (packed) weights; a fixture is valid
only when that headroom is positive on every element and every stored non-zero value is a normal number of the dtype.

The construction.  One layer under test gets dense small-integer weights (``with_dense``); every other layer is a selector
(``selector_state_dict``): each output channel copies one input channel at one tap.  Frames are k / 256, so what reaches the
layer under test are single input pixels plus a few bias steps of 2^-8 (sums of two at a residual).

Rounding points of the 16-bit paths (tools/bf16_budget.py): every packed GEMM weight and every activation
that is stored or handed to an MFMA; accumulation, bias, activation functions and residual adds are f32; depthwise weights
and the stem stay f32.  Stage outputs are f32; their copy in the concat buffer is 16-bit.

ELU's negative branch (a polynomial / the hardware exponential) is not exact: the fixtures above keep every ELU operand >= 0,
which ``exactness`` checks, and the ``elu:*`` fixtures at the end of this file pin the branch by a derived bound instead:
an exactly known negative operand per element, fp32 within 1e-6 relative of float64 expm1, bf16 / fp16 within one step of the
format + 2^-22 of the rounded expm1 (which says nothing below |z| of about 2^-22, where the 16-bit form cancels).  The
dw<px=2> kernel runs every depthwise fixture through LWP_DW_PX=2 (tests/variant_matrix.py).

fp16 subnormals: the ``f16sub:*`` fixtures (bit exact like the others; plain fixtures at fp32 and bf16) store and consume
values below 2^-14 at fp16 in every kernel family: gradual underflow, round to nearest even on the subnormal grid, no flush.

fp16 overflow: the ``f16ovf:*`` fixtures (again plain exact fixtures at fp32 and bf16) store 65504, values in (65504, 65520),
the tie 65520 and larger values at fp16 in every kernel family and read one consumer behind them: round to nearest even to
inf, no saturation; inf x 0 is NaN and stays NaN through ReLU, as in the float64 reference.
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import lwpose_amd  # noqa: F401
from lwpose_amd import synth
from lwpose_amd.arch import BACKBONE, param_table

DTYPES = ("fp32", "bf16", "fp16")
FRAMES = [(2, 91, 149), (1, 91, 149)]        # variant_matrix.FRAME (M = 456 at stride 8) and its batch-1 form (M = 228)
VAR = np.float32(1.0 - 1e-5)                  # running_var of every BatchNorm: gamma / sqrt((double)var + 1e-5) is gamma to 7e-9
# dense entries with 9 to 12 significant bits, in units of the layer's weight step: ties of the 8-bit significand (257 -> 256,
# 259 -> 260, 261 -> 260 under round-to-nearest-even; truncation and ties-away give other values), a non-tie (1027) and ties of
# the 11-bit significand (2049 -> 2048, 2051 -> 2052)
SPECIALS = (257, -259, 1027, 2049, -2051, 261)
# where the residual adds of the refinement blocks have used the bits up (blocks 1..4 and the refinement heads): the 9-bit ones only
SPECIALS9 = (257, -259, 261)


# ------------------------------------------------------------------------------------------------------------ frames
def frame(shape, seed=7):
    """(N, 3, H, W) float32, values k / 256 with k integer in [-128, 127]."""
    n, h, w = shape
    k = (synth.splitmix64(np.arange(n * 3 * h * w, dtype=np.uint64), synth.fnv1a64("exact-frame", seed)) >> np.uint64(24)) % np.uint64(256)
    return ((k.astype(np.int64) - 128).astype(np.float32) / np.float32(256)).reshape(n, 3, h, w)


# ------------------------------------------------------------------------------------------------------------ weights
def _bn_of(conv_key):
    """BatchNorm that follows a conv in the state dict (None: the conv has none)."""
    p = conv_key.split(".")
    if p[0] == "model":
        return "model.%s.%d" % (p[1], int(p[2]) + 1)
    if p[0] == "refinement_stages" and p[-3] == "trunk" and p[-1] == "0" and p[-2] in ("0", "1") and len(p) == 7:
        return ".".join(p[:-1]) + ".1"
    return None


def _hash(key, seed, n):
    return synth.splitmix64(np.arange(n, dtype=np.uint64), synth.fnv1a64(key, seed))


# Shifted copies of one frame can coincide (a stem tap one row down, read one row up, is the same pixels), and two equal input
# channels would hide a permutation of K between them.  The selectors named here draw their choice from a later stream of the
# generator (seed 1); tests/test_exact_host.py checks that the channels of every tensor a layer under test reads are distinct.
REDRAW = {"model.1.0": 1, "initial_stage.heatmaps.1.0": 19, "initial_stage.pafs.1.0": 19, "refinement_stages.0.heatmaps.1.0": 5,
          "refinement_stages.0.pafs.1.0": 5, "refinement_stages.1.trunk.0.initial.0": 2, "refinement_stages.1.heatmaps.1.0": 1,
          "refinement_stages.1.pafs.1.0": 1}


def _draw(conv, what, seed, n):
    r = REDRAW.get(conv, 0) if seed == 1 else 0
    return _hash(conv + what + (":%d" % r if r else ""), seed, n)


def selector_state_dict(nref=1, seed=1):
    """A full state dict (synth.make_state_dict's format) in which every conv output channel has exactly one non-zero weight.

    A 3x3 picks (input channel, tap) and a 1x1 its input channel through a pseudo-random permutation, so no two outputs of a
    layer copy the same thing until the choices run out (the stem: 27 for 32 outputs; a 1x1 that widens); those repeats get a
    bias a few steps of 2^-8 apart, or a gain 1, 1/2, 1/4, 1/8 in the first head convs (initial stage: 512 from 128), which the second head conv undoes, so that the stage outputs are on the 2^-8 grid again.  The entry
    1x1 of refinement blocks 1..4 has gain 1/2, which keeps the residual sums from doubling per block.  Biases are small
    multiples of 2^-8; BatchNorm: var = float32(1 - 1e-5), gamma 1 (2 on a few channels of two depthwise layers), mean and beta multiples of
    2^-8 that never cancel (so that the fold's 7e-9 relative error cannot leave a tiny non-zero bias)."""
    sd = OrderedDict()
    table = param_table(nref)
    has_bias = {p.key[:-5] for p in table if p.role == "conv_b"}
    repeat = {}
    for p in table:
        if p.role != "conv_w":
            continue
        conv = p.key[:-7]
        co, cig, k, _ = p.shape
        w = np.zeros(p.shape, np.float32)
        rep = np.zeros(co, np.int64)
        if cig == 1 and co > 3:                                   # depthwise: a tap per channel
            tap = (_draw(conv, "/tap", seed, co) % np.uint64(9)).astype(np.int64)
            w.reshape(co, 9)[np.arange(co), tap] = 1.0
        else:
            n = cig * k * k
            perm = np.argsort(_draw(conv, "/perm", seed, n), kind="stable")
            o = np.arange(co)
            pick = perm[o % n]
            rep = o // n
            gain = np.ones(co, np.float32)
            if conv.endswith(".heatmaps.0.0") or conv.endswith(".pafs.0.0"):
                gain = np.float32(2.0) ** (-rep).astype(np.float32)
                rep = np.zeros(co, np.int64)
            elif conv.endswith(".initial.0") and ".trunk.0.initial" not in conv:
                gain = np.full(co, 0.5, np.float32)
            elif conv.endswith(".heatmaps.1.0") or conv.endswith(".pafs.1.0"):
                # undoes the gain of the hidden channel it copies; the 2 keeps a stage map, a shifted copy of some feature
                # channel like everything here, from being equal to a channel of the features it is concatenated with
                gain = np.float32(2.0) ** (1 + pick // 128).astype(np.float32)
            w.reshape(co, n)[o, pick] = gain
        repeat[conv] = rep
        sd[p.key] = w
    for p in table:
        if p.role == "conv_w":
            continue
        if p.role == "bn_nbt":
            sd[p.key] = np.array(1, dtype=np.int64)
            continue
        c = p.shape[0]
        if p.role == "conv_b":
            conv = p.key[:-5]
            k = (_hash(p.key, seed, c) % np.uint64(4) == 0).astype(np.int64)
            if _bn_of(conv) is None:
                k = k + 2 * repeat[conv]                        # beyond what the random step can reach: repeats stay distinct
            sd[p.key] = (k.astype(np.float32) / np.float32(256))
            continue
        bn = p.key.rsplit(".", 1)[0]
        conv = bn.rsplit(".", 1)[0] + ".%d" % (int(bn.rsplit(".", 1)[1]) - 1)
        rep = repeat[conv]
        sign = np.where((_hash(bn + "/sign", seed, c) & np.uint64(1)).astype(np.int64) == 1, -1, 1)
        sign = np.where(rep > 0, 1, sign)
        a = (_hash(bn + "/a", seed, c) % np.uint64(4) == 0).astype(np.int64)      # (conv bias - mean) = sign * a / 256
        b = (_hash(bn + "/b", seed, c) % np.uint64(4) == 1).astype(np.int64)      # beta = sign * b / 256 (+ the repeat step)
        if p.role == "bn_var":
            v = np.full(c, VAR, np.float32)
        elif p.role == "bn_w":
            v = np.ones(c, np.float32)
            if conv in ("model.3.0", "model.8.0"):
                v = np.where(_hash(bn + "/gamma", seed, c) % np.uint64(16) == 0, np.float32(2), np.float32(1)).astype(np.float32)
        elif p.role == "bn_mean":
            cb = sd[conv + ".bias"].astype(np.float64) * 256 if conv in has_bias else np.zeros(c)
            v = ((cb - sign * a) / 256.0).astype(np.float32)
        else:
            v = ((sign * b + 4 * rep) / 256.0).astype(np.float32)
        sd[p.key] = v
    return OrderedDict((p.key, torch.from_numpy(np.ascontiguousarray(sd[p.key])).reshape(p.shape)) for p in table)


def with_dense(sd, convs, seed=1, opts=None):
    """A copy of ``sd`` (untouched entries shared) with the named convs' weights replaced by dense integers times 2^-2.

    Integers are pseudo-random in {-2, -1, 1, 2}: both signs, distinct per tap, asymmetric in (o, ci).  Per conv, ``opts`` may
    set ``maxint`` (1: {-1, 1}), ``nonneg`` (ELU layers: {1, 2}, so that ELU stays on its identity branch), ``keep`` (one in
    ``keep`` entries stays non-zero; ``neg_one_in``: one entry in so many is negative: the joint cpm trunk fixture, whose non-negative chain has no cancellation) and
    ``specials`` (default on; a tuple replaces SPECIALS): six entries in six different rows carry SPECIALS, 9 to 12 significant
    bits with exact ties of the 8-bit and 11-bit significand, which pins the packer's round-to-nearest-even narrowing.  The
    depthwise and stem weights stay f32 on every path, so there the same entries give products of 17 to 20 bits, and the
    16-bit store after them has to round."""
    out = OrderedDict(sd)
    opts = opts or {}
    for conv in convs:
        o_ = dict(maxint=2, nonneg=False, keep=1, specials=True, step=0.25, neg_one_in=2)
        o_.update(opts.get(conv, {}))
        w0 = sd[conv + ".weight"]
        co, cig, k, _ = w0.shape
        n = co * cig * k * k
        h = _hash(conv + "/dense", seed, n)
        mag = ((h >> np.uint64(8)) % np.uint64(o_["maxint"])).astype(np.int64) + 1
        sgn = np.where((h >> np.uint64(20)) % np.uint64(o_["neg_one_in"]) == 0, -1, 1)
        v = mag if o_["nonneg"] else mag * sgn
        if o_["keep"] > 1:
            v = np.where((h >> np.uint64(32)) % np.uint64(o_["keep"]) == 0, v, 0)
        v = v.reshape(co, cig * k * k).astype(np.float64)
        # one positive entry in every row: a row of negative (or no) weights is zero behind its ReLU, and two zero channels
        # would be equal inputs of the next layer under test
        v[np.arange(co), (_hash(conv + "/pos", seed, co) % np.uint64(cig * k * k)).astype(np.int64)] = 1
        depthwise = cig == 1 and co > 3
        if o_["specials"]:
            sp = SPECIALS if o_["specials"] is True else o_["specials"]
            hs = _hash(conv + "/special", seed, 2 * len(sp))
            rows = np.argsort(_hash(conv + "/rows", seed, co), kind="stable")[:len(sp)]
            for i, s in enumerate(sp):
                v[rows[i], int(hs[2 * i] % np.uint64(cig * k * k))] = abs(s) if o_["nonneg"] else s
        out[conv + ".weight"] = torch.from_numpy((v * o_["step"]).astype(np.float32).reshape(tuple(w0.shape)))
    return out


# ------------------------------------------------------------------------------------------------------------ rounding
def _r_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _r_f16(t):
    return t.to(torch.float32).to(torch.float16).to(torch.float64)


def _trunc(bits):
    def f(t):
        u = t.to(torch.float32).contiguous().view(torch.int32)
        return (u & ~((1 << bits) - 1)).view(torch.float32).to(torch.float64)
    return f


ROUND = {"fp32": lambda t: t, "bf16": _r_bf16, "fp16": _r_f16}
TRUNCATE = {"bf16": _trunc(16), "fp16": _trunc(13)}     # round-towards-zero of a normal number (the fault a fixture must bite on)
NORMAL = {"fp32": (2.0 ** -126, 3.4e38), "bf16": (2.0 ** -126, 3.38e38), "fp16": (2.0 ** -14, 65504.0)}


def _lowbit(t):
    """Smallest set bit (as a power of two) over the non-zero entries of a float64 tensor; inf if all are zero."""
    a = t.detach().numpy().ravel()
    a = a[(a != 0) & np.isfinite(a)]
    if a.size == 0:
        return float("inf")
    m, e = np.frexp(np.abs(a))
    mi = (m * 2.0 ** 53).astype(np.int64)
    return float(np.min(np.ldexp((mi & -mi).astype(np.float64), e - 53)))


def fold(sd, conv, bn):
    """(weight, bias) of a conv with its BatchNorm folded as the packer does: double arithmetic, one rounding to f32."""
    w = sd[conv + ".weight"].double()
    b = sd[conv + ".bias"].double() if conv + ".bias" in sd else torch.zeros(w.shape[0], dtype=torch.float64)
    if bn:
        sc = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
        w = w * sc.view(-1, 1, 1, 1)
        b = (b - sd[bn + ".running_mean"].double()) * sc + sd[bn + ".bias"].double()
    return w.float().double(), b.float().double()


# ------------------------------------------------------------------------------------------------------------ reference
class _Stop(Exception):
    pass


def reference(sd, x, nref=1, dtype="fp32", base=None, round16=None, stop_after=None, probe=False):
    """{engine layer name: float64 array}: the network in float64, rounded exactly where the ``dtype`` path rounds.

    Names are the engine's: "model.N.pw" (and "model.N.dw", the depthwise result: in memory only in the unfused fp32 graph),
    "cpm.trunk.J.pw" (J = 2: with the residual, what the layer stores), "P.heads.0" / "P.heads.1" ([heat | paf]; heads.1 is
    the f32 stage output, "P.heads.1.cat" its 16-bit copy in the concat buffer), "Q.initial", "Q.trunk.0", "Q.trunk.1" (the
    block output).  ``base`` = (state dict, result) of an earlier call on the same input, dtype and rounding: layers up to the
    first one whose parameters differ are taken from it.  ``round16`` replaces the dtype's rounding (tests flip it to
    truncation).  ``probe``: also record, under "_exact", per reduction (headroom bits, smallest ELU operand) and under
    "_stored" per rounding point (smallest, largest non-zero stored magnitude) and under "_z" the operand tensor of every ELU."""
    h16 = dtype != "fp32"
    r16 = round16 or ROUND[dtype]
    taps, exact, stored, zs = OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()
    st = {"dirty": base is None, "elu_min": float("inf")}
    x = torch.as_tensor(np.asarray(x)).double()

    def note_stored(name, t):
        if probe:
            a = t.abs()
            nz = a[a != 0]
            lo, hi = (float(nz.min()), float(nz.max())) if nz.numel() else (float("inf"), 0.0)
            old = stored.get(name, (float("inf"), 0.0))
            stored[name] = (min(lo, old[0]), max(hi, old[1]))

    def A(name, t):                                       # an activation that is stored / handed to an MFMA
        t = r16(t) if h16 else t
        note_stored(name, t)
        return t

    def conv(name, xin, ck, bn=None, stride=1, pad=0, dil=1, groups=1, gemm=True):
        w, b = fold(sd, ck, bn)
        if gemm and h16:
            w = r16(w)
            note_stored(name + "/w", w)
        y = F.conv2d(xin, w, b, stride, pad, dil, groups)
        if probe:
            xf = torch.where(torch.isfinite(xin), xin, torch.zeros_like(xin))        # (the f16ovf fixtures: the finite part)
            s = float(F.conv2d(xf.abs(), w.abs(), b.abs(), stride, pad, dil, groups).max())
            q = min(_lowbit(xf) * _lowbit(w), _lowbit(b))
            exact[name] = 24.0 - float(np.log2(s / q)) if s > 0 and np.isfinite(q) else 24.0
        return y

    def add(name, a, b):                                  # f32 residual add in an epilogue
        if probe:
            s, q = float((a.abs() + b.abs()).max()), min(_lowbit(a), _lowbit(b))
            exact[name] = 24.0 - float(np.log2(s / q)) if s > 0 and np.isfinite(q) else 24.0
        return a + b

    def elu(name, t):
        if probe:
            exact[name + "/elu_min"] = float(t[torch.isfinite(t)].min())      # (the f16ovf fixtures: of the finite operands)
            zs[name] = t                                  # the ELU's operand, element by element (the bounded ELU fixtures)
        return F.elu(t)

    def keys(ck, bn=None):
        ks = [ck + ".weight", ck + ".bias"]
        if bn:
            ks += [bn + s for s in (".weight", ".bias", ".running_mean", ".running_var")]
        return [k for k in ks if k in sd]

    def step(names, ks, fn):
        """Run ``fn`` (-> tensors for ``names``) unless nothing up to here differs from ``base``."""
        if not st["dirty"] and all(sd[k] is base[0][k] for k in ks) and all(n in base[1] for n in names):
            for n in names:
                taps[n] = base[1][n]
            for src, dst in ((base[1].get("_exact", {}), exact), (base[1].get("_stored", {}), stored), (base[1].get("_z", {}), zs)):
                for k, v in src.items():
                    if k.split("/")[0] in names:
                        dst[k] = v
        else:
            st["dirty"] = True
            vals = fn()
            for n, v in zip(names, vals):
                taps[n] = v
        if stop_after in names:
            raise _Stop
        return [taps[n] for n in names]

    def heads(t, p):
        ks = sum([keys(p + ".%s.%d.0" % (nm, i)) for nm in ("heatmaps", "pafs") for i in (0, 1)], [])

        def fn():
            hid = [A(p + ".heads.0", F.relu(conv(p + ".heads.0/" + nm, t, p + "." + nm + ".0.0"))) for nm in ("heatmaps", "pafs")]
            out = [conv(p + ".heads.1/" + nm, hd, p + "." + nm + ".1.0") for nm, hd in zip(("heatmaps", "pafs"), hid)]
            cat = [A(p + ".heads.1.cat", o) for o in out]
            return torch.cat(hid, 1), torch.cat(out, 1), torch.cat(cat, 1)
        return step([p + ".heads.0", p + ".heads.1", p + ".heads.1.cat"], ks, fn)

    try:
        with torch.no_grad():
            (t,) = step(["model.0"], keys("model.0.0", "model.0.1"),
                        lambda: [A("model.0", F.relu(conv("model.0", x, "model.0.0", "model.0.1", 2, 1, gemm=False)))])
            for i, (cin, cout, s, d) in enumerate(BACKBONE, start=1):
                n_dw, n_pw = "model.%d.dw" % i, "model.%d.pw" % i
                (t,) = step([n_dw], keys("model.%d.0" % i, "model.%d.1" % i), lambda: [
                    A(n_dw, F.relu(conv(n_dw, t, "model.%d.0" % i, "model.%d.1" % i, s, d, d, cin, gemm=False)))])
                (t,) = step([n_pw], keys("model.%d.3" % i, "model.%d.4" % i), lambda: [
                    A(n_pw, F.relu(conv(n_pw, t, "model.%d.3" % i, "model.%d.4" % i)))])
            (a,) = step(["cpm.align"], keys("cpm.align.0"), lambda: [A("cpm.align", F.relu(conv("cpm.align", t, "cpm.align.0")))])
            t = a
            for j in range(3):
                n_dw, n_pw = "cpm.trunk.%d.dw" % j, "cpm.trunk.%d.pw" % j
                (t,) = step([n_dw], keys("cpm.trunk.%d.0" % j), lambda: [
                    A(n_dw, elu(n_dw, conv(n_dw, t, "cpm.trunk.%d.0" % j, None, 1, 1, 1, t.shape[1], gemm=False)))])

                def pw():
                    u = elu(n_pw, conv(n_pw, t, "cpm.trunk.%d.2" % j))
                    return [A(n_pw, add(n_pw + "/res", u, a) if j == 2 else u)]
                (t,) = step([n_pw], keys("cpm.trunk.%d.2" % j), pw)
            (feat,) = step(["cpm.conv"], keys("cpm.conv.0"), lambda: [A("cpm.conv", F.relu(conv("cpm.conv", t, "cpm.conv.0", None, 1, 1)))])
            t = feat
            for j in range(3):
                nm = "initial_stage.trunk.%d" % j
                (t,) = step([nm], keys(nm + ".0"), lambda: [A(nm, F.relu(conv(nm, t, nm + ".0", None, 1, 1)))])
            _, _, cat = heads(t, "initial_stage")
            for k in range(nref):
                p = "refinement_stages.%d" % k
                t = torch.cat([feat, cat], 1)
                for bl in range(5):
                    q = "%s.trunk.%d" % (p, bl)
                    (ini,) = step([q + ".initial"], keys(q + ".initial.0"), lambda: [
                        A(q + ".initial", F.relu(conv(q + ".initial", t, q + ".initial.0")))])
                    (u,) = step([q + ".trunk.0"], keys(q + ".trunk.0.0", q + ".trunk.0.1"), lambda: [
                        A(q + ".trunk.0", F.relu(conv(q + ".trunk.0", ini, q + ".trunk.0.0", q + ".trunk.0.1", 1, 1)))])
                    (t,) = step([q + ".trunk.1"], keys(q + ".trunk.1.0", q + ".trunk.1.1"), lambda: [
                        A(q + ".trunk.1", add(q + ".trunk.1/res", F.relu(conv(q + ".trunk.1", u, q + ".trunk.1.0", q + ".trunk.1.1", 1, 2, 2)), ini))])
                _, _, cat = heads(t, p)
    except _Stop:
        pass
    out = OrderedDict((k, v.numpy()) for k, v in taps.items())
    res = _Result(out)
    res.tensors = taps
    if probe:
        res["_exact"], res["_stored"], res["_z"] = exact, stored, zs
    return res


class _Result(OrderedDict):
    """reference()'s result; ``base`` reuse reads the tensors back through item access."""
    tensors = None


def as_base(sd, res):
    """(sd, {name: tensor}) for ``reference(base=...)``."""
    d = dict(res.tensors)
    for k in ("_exact", "_stored", "_z"):
        if k in res:
            d[k] = res[k]
    return sd, d


# ------------------------------------------------------------------------------------------------------------ fixtures
def layer_of(conv):
    """Engine layer (default graph: fused depthwise + pointwise, merged head pairs) that runs a conv of the state dict."""
    p = conv.split(".")
    if p[0] == "model":
        return "model.0" if p[1] == "0" else "model.%s.pw" % p[1]
    if p[0] == "cpm" and p[1] == "trunk":
        return "cpm.trunk.%s.pw" % p[2]
    if p[-3] in ("heatmaps", "pafs"):
        return ".".join(p[:-3]) + ".heads." + p[-2]
    return conv[:-2]


def reductions_of(conv):
    """Names under which ``reference`` records the reductions of a conv (its own and the residual add of its epilogue)."""
    p = conv.split(".")
    if p[0] == "model" and p[1] != "0":
        return ["model.%s.%s" % (p[1], "dw" if p[2] == "0" else "pw")]
    if p[0] == "cpm" and p[1] == "trunk":
        nm = "cpm.trunk.%s.%s" % (p[2], "dw" if p[3] == "0" else "pw")
        return [nm, nm + "/res"] if nm == "cpm.trunk.2.pw" else [nm]
    if p[-3] in ("heatmaps", "pafs"):
        return [layer_of(conv) + "/" + p[-3]]
    nm = layer_of(conv)
    return [nm, nm + "/res"] if nm.startswith("refinement_stages.") and nm.endswith(".trunk.1") and nm.count(".trunk.") == 2 else [nm]


def _fixture(name, convs, nref=1, opts=None, joint=False, seed=1):
    layers = []
    for c in convs:
        if layer_of(c) not in layers:
            layers.append(layer_of(c))
    if layers[-1].endswith(".heads.0"):          # alone the first head pair runs as a plain GEMM; the fused pair's kernel shows in heads.1
        layers.append(layers[-1][:-1] + "1")
    return dict(name=name, convs=list(convs), nref=nref, opts=opts or {}, joint=joint, layers=layers, seed=seed)


def _conv_keys(nref):
    return [p.key[:-7] for p in param_table(nref) if p.role == "conv_w"]


def _elu(conv):
    return conv.startswith("cpm.trunk.")


def build_fixtures():
    fx = []
    # one per conv of the nref = 1 network
    for c in _conv_keys(1):
        deep = c.startswith("refinement_stages.") and ".trunk.0." not in c[:len("refinement_stages.0.trunk.0.")]
        fx.append(_fixture(c, [c], opts={c: dict(nonneg=True)} if _elu(c) else {c: dict(specials=SPECIALS9)} if deep else None))
    # one per group a kernel fuses, all members dense together; the second reduction of a chain sees the first's sums, so its
    # integers are +-1 (the budget: sum|t| / q < 2^24)
    for i in range(1, 12):
        dw, pw = "model.%d.0" % i, "model.%d.3" % i
        fx.append(_fixture("model.%d.dw+pw" % i, [dw, pw], opts={dw: dict(specials=False), pw: dict(maxint=1)}, joint=True))
    for j in range(3):
        dw, pw = "cpm.trunk.%d.0" % j, "cpm.trunk.%d.2" % j
        fx.append(_fixture("cpm.trunk.%d.dw+pw" % j, [dw, pw], opts={dw: dict(nonneg=True, specials=False), pw: dict(nonneg=True, keep=2)}, joint=True))
    for p in ("initial_stage", "refinement_stages.0"):
        cs = [p + ".heatmaps.0.0", p + ".pafs.0.0", p + ".heatmaps.1.0", p + ".pafs.1.0"]
        o = {c: dict(maxint=1, keep=4 if p == "initial_stage" else 8, step=1.0, specials=SPECIALS9 if c.endswith(".1.0") else False) for c in cs}
        if p != "initial_stage":               # its input is >= 0 everywhere: with half the sparse entries negative some hidden channels are zero
            for c in cs[:2]:
                o[c]["neg_one_in"] = 4
        fx.append(_fixture(p + ".heads.0+1", cs, opts=o, joint=True))
    for bl in range(4):
        a, b = "refinement_stages.0.trunk.%d.trunk.1.0" % bl, "refinement_stages.0.trunk.%d.initial.0" % (bl + 1)
        fx.append(_fixture("refinement_stages.0.trunk.%d.trunk.1+1x1" % bl, [a, b], opts={a: dict(specials=False, maxint=1, keep=32, step=1.0), b: dict(maxint=1, keep=8, step=1.0, specials=SPECIALS9)}, joint=True))
    # the cpm trunk as one kernel: six non-negative reductions in a row, no cancellation, so one entry in `keep` stays
    cs = [c for j in range(3) for c in ("cpm.trunk.%d.0" % j, "cpm.trunk.%d.2" % j)]
    o = {c: dict(nonneg=True, maxint=1, specials=False, keep=3 if c.endswith(".0") else 32, step=1.0 if c.endswith(".0") else 0.5) for c in cs}
    fx.append(_fixture("cpm.trunk.all", cs, opts=o, joint=True))
    # concat copies of later stages: an nref = 3 selector net with the dense layer in stage 2
    c = "refinement_stages.1.trunk.0.initial.0"
    fx.append(_fixture("nref3:" + c, [c], nref=3))
    return fx


# ------------------------------------------------------------------------------------------------------------ fp16 subnormals
# Plain exact fixtures at fp32 and bf16; at fp16 the stored activations of the layers between ``down`` and ``up`` are subnormal
# (the "stored values are normal" rule is lifted for them at fp16 only: ``subnormal_ok``), and the oracle is torch's CPU half
# rounding: IEEE gradual underflow, round to nearest even.  ``down`` (one or two convs) is scaled by 2^-17, so what it stores
# are the multiples n 2^-25 of HALF the subnormal spacing: odd n are exact ties (3 -> 4 rounds to even upwards, 5 -> 4 downwards,
# 1 -> 0 is a non-zero value that rounds to 0); its bias, which is what a pixel with a zero input stores, cycles through
# F16SUB_BIAS: 2^-24, the ties, the largest subnormal 1023 2^-24 and the smallest normal 2^-14.  The convs in ``mid`` lose
# their bias (it would be 2^17 times too large) and pass the subnormals on: depthwise unpack, MFMA activation operand, residual
# and concat copies.  ``up`` multiplies by 2^13 (2^16 is no fp16 weight), back to normal numbers k 2^-12: the subnormals are
# consumed and not only stored.  2^-17 is itself a subnormal packed GEMM weight where ``down`` is a GEMM.
F16SUB_DOWN, F16SUB_UP = 2.0 ** -17, 2.0 ** 13
F16SUB_BIAS = (0, 2, 1, 3, 5, 7, 2046, 2048)          # in units of 2^-25
F16SUB = [
    dict(name="model.0>model.1", down=["model.0.0"], mid=[], up="model.1.0"),                    # stem store -> depthwise unpack
    dict(name="model.1>model.2", down=["model.1.3"], mid=[], up="model.2.0"),                    # fused block store -> stride-2 depthwise
    dict(name="model.4>model.5", down=["model.4.3"], mid=[], up="model.5.0"),
    dict(name="model.6>model.7", down=["model.6.3"], mid=[], up="model.7.0"),                    # 512 outputs -> dilation 2
    dict(name="model.5.dw>pw", down=["model.5.0"], mid=[], up="model.5.3"),                      # a 2^-17 f32 tap: subnormal MFMA operand inside one kernel
    dict(name="cpm", down=["cpm.align.0"], mid=["cpm.trunk.%d.%d" % (j, k) for j in range(3) for k in (0, 2)], up="cpm.conv.0"),
    # feature and stage maps both subnormal: the f32 stage outputs stay normal f32 numbers, their 16-bit concat copy is subnormal
    dict(name="cpm.conv>concat", down=["cpm.conv.0"],
         mid=["initial_stage.trunk.%d.0" % j for j in range(3)] + ["initial_stage.%s.%d.0" % (n, k) for k in (0, 1) for n in ("heatmaps", "pafs")],
         up="refinement_stages.0.trunk.0.initial.0"),
    dict(name="refinement", down=["refinement_stages.0.trunk.0.initial.0"],
         mid=["refinement_stages.0.trunk.0.trunk.0.0", "refinement_stages.0.trunk.0.trunk.1.0"], up="refinement_stages.0.trunk.1.initial.0"),
]


def _set(out, key, arr, like):
    out[key] = torch.from_numpy(np.ascontiguousarray(np.asarray(arr, np.float32))).reshape(tuple(like.shape))


def f16sub_state_dict(sd, spec, down=None, up=None, bias=None):
    """``spec``'s ``down`` convs scaled by ``down`` (a power of two, or one per output channel) with the folded bias
    ``bias(co)``, its ``mid`` convs without bias, its ``up`` conv scaled by ``up`` (defaults: the f16sub values)."""
    out = OrderedDict(sd)
    down = F16SUB_DOWN if down is None else down
    up = F16SUB_UP if up is None else up
    bias = bias or (lambda co: np.asarray(F16SUB_BIAS, np.float64)[np.arange(co) % len(F16SUB_BIAS)] * 2.0 ** -25)

    def rebias(conv, scale, bias):
        """Scale the conv's output by ``scale`` and make its (folded) bias ``bias``."""
        w = sd[conv + ".weight"]
        bn = _bn_of(conv)
        if bn:
            cb = sd[conv + ".bias"].numpy() if conv + ".bias" in sd else np.zeros(w.shape[0], np.float32)
            _set(out, bn + ".weight", sd[bn + ".weight"].numpy() * np.asarray(scale, np.float32), sd[bn + ".weight"])
            _set(out, bn + ".running_mean", cb, sd[bn + ".running_mean"])
            _set(out, bn + ".bias", bias, sd[bn + ".bias"])
        else:
            _set(out, conv + ".weight", w.numpy() * np.asarray(scale, np.float32).reshape(-1, 1, 1, 1), w)
            if conv + ".bias" in sd:
                _set(out, conv + ".bias", bias, sd[conv + ".bias"])
    for conv in spec["down"]:
        co = sd[conv + ".weight"].shape[0]
        rebias(conv, down(co) if callable(down) else down, bias(co))
    for conv in spec["mid"]:
        rebias(conv, 1.0, np.zeros(sd[conv + ".weight"].shape[0]))
    _set(out, spec["up"] + ".weight", sd[spec["up"] + ".weight"].numpy() * np.float32(up), sd[spec["up"] + ".weight"])
    return out


def build_f16sub_fixtures():
    fx = []
    for spec in F16SUB:
        f = _fixture("f16sub:" + spec["name"], spec["down"] + spec["mid"] + [spec["up"]])
        f.update(f16sub=spec, subnormal_ok=True)
        fx.append(f)
    return fx


F16SUB_FIXTURES = build_f16sub_fixtures()


# ------------------------------------------------------------------------------------------------------------ fp16 overflow
# Plain exact fixtures at fp32 and bf16 (65520 is a finite number there); at fp16 the oracle is torch's CPU half rounding:
# round to nearest even to inf, no saturation.  ``down`` is scaled by 2^5, so it stores k 2^-3 with k < 532, and one channel
# gets the bias 65504 and one 65512 on top (``_ovf_channels`` picks them by the selector network's batch-1 activations): a pixel with a zero input stores 65504 (or 65512, which rounds to 65504), small
# inputs land in (65504, 65520) and round to 65504, 65504 + 16 and 65512 + 8 are the tie 65520, which rounds to even = inf,
# and everything above is inf.  The stage heads have no ReLU: there two more channels are the same, negated (weight and bias),
# which gives the negative twins; the f32 stage outputs stay finite while their 16-bit concat copy is +-inf.  ``up`` (the only
# consumer that is read) multiplies by 2^-5: inf stays inf, and inf x 0, a zero weight or tap on an inf, is NaN, in the float64
# reference as on the device; ``check`` treats NaN at the same place and inf of the same sign as equal for these fixtures only.
F16OVF_UP, F16OVF_DOWN = 2.0 ** 5, 2.0 ** -5
F16OVF = [
    dict(name="model.0>model.1", down=["model.0.0"], mid=[], up="model.1.0"),
    dict(name="model.1>model.2", down=["model.1.3"], mid=[], up="model.2.0"),
    dict(name="model.4>model.5", down=["model.4.3"], mid=[], up="model.5.0"),
    dict(name="model.6>model.7", down=["model.6.3"], mid=[], up="model.7.0"),
    dict(name="model.5.dw>pw", down=["model.5.0"], mid=[], up="model.5.3"),
    dict(name="cpm.align>trunk", down=["cpm.align.0"], mid=[], up="cpm.trunk.0.0"),
    dict(name="cpm.conv>trunk", down=["cpm.conv.0"], mid=[], up="initial_stage.trunk.0.0"),
    dict(name="heads>concat", down=["initial_stage.heatmaps.1.0", "initial_stage.pafs.1.0"], mid=[], up="refinement_stages.0.trunk.0.initial.0", twins=True),
    dict(name="refinement", down=["refinement_stages.0.trunk.0.initial.0"], mid=[], up="refinement_stages.0.trunk.0.trunk.0.0"),
    dict(name="refinement.3x3>3x3", down=["refinement_stages.0.trunk.0.trunk.0.0"], mid=[], up="refinement_stages.0.trunk.0.trunk.1.0"),
    # (the 1x1 that the window-resident 3x3 in front of it can carry in its epilogue)
    dict(name="refinement.1", down=["refinement_stages.0.trunk.1.initial.0"], mid=[], up="refinement_stages.0.trunk.1.trunk.0.0"),
]


def _first_tensor(spec):
    """reference() name of the tensor the first ``down`` conv of an f16sub / f16ovf spec writes."""
    c = spec["down"][0]
    p = c.split(".")
    return "model.%s.dw" % p[1] if p[0] == "model" and p[1] != "0" and p[2] == "0" else layer_of(c)


def _ovf_channels(y, twins):
    """Channels of ``y`` (N, C, H, W; the scaled tensor without the special bias, multiples of 2^-3) for the biases 65504, 65512
    (and, with ``twins``, -65504, -65512): the first holds 0, values in (0, 16), 16 (65504 + 16 is the tie 65520) and more,
    the second 8 (65512 + 8 is that tie again)."""
    rows = y.transpose(1, 0, 2, 3).reshape(y.shape[1], -1)
    ok = [c for c, r in enumerate(rows) if (r == 0).any() and ((r > 0) & (r < 16)).any()]
    full = [c for c in ok if (rows[c] == 16).any() and (rows[c] > 16).any()] or ok       # (the stem's scaled values end below 16)
    rest = [c for c in range(len(rows)) if c not in full[:2] and (rows[c] > 8).any()]
    half = [c for c in rest if (rows[c] == 8).any()] or [c for c in rest if (rows[c] == 0).any()]
    need = 2 if twins else 1
    assert len(full) >= need and len(half) >= need, (len(full), len(half))
    return [full[0], half[0]] + ([full[1], half[1]] if twins else [])


def f16ovf_state_dict(sd, spec):
    tw = bool(spec.get("twins"))
    big = spec.get("scale", F16OVF_UP)
    plain = f16sub_state_dict(sd, spec, down=big, up=1.0, bias=lambda co: np.zeros(co))
    y = reference(plain, frame_of(FRAMES[1]), 1, "fp32", base=selector_run(FRAMES[1], "fp32"), stop_after=layer_of(spec["down"][0]))[_first_tensor(spec)]
    at, chosen = 0, {}
    for conv in spec["down"]:                              # (the two head convs write one tensor: [heat | paf])
        co = sd[conv + ".weight"].shape[0]
        chosen[co] = _ovf_channels(y[:, at:at + co], tw)
        at += co

    def sign(co):
        v = np.ones(co)
        v[chosen[co][2:]] = -1.0
        return v

    def bias(co):
        v = np.zeros(co)
        v[chosen[co][0::2]], v[chosen[co][1::2]] = 65504.0, 65512.0
        return v * sign(co)
    return f16sub_state_dict(sd, spec, down=lambda co: big * sign(co), up=1.0 / big, bias=bias)


def build_f16ovf_fixtures():
    fx = []
    for spec in F16OVF:
        f = _fixture("f16ovf:" + spec["name"], spec["down"] + [spec["up"]])
        f.update(f16ovf=spec, nonfinite_ok=True)
        fx.append(f)
    return fx


F16OVF_FIXTURES = build_f16ovf_fixtures()
FIXTURES = build_fixtures()
ALL_EXACT = FIXTURES + F16SUB_FIXTURES + F16OVF_FIXTURES        # everything that is compared bit for bit on the device
BY_NAME = {f["name"]: f for f in ALL_EXACT}


def fixtures_for(layer, nref=1):
    """Fixtures whose layers under test include engine layer ``layer`` ("model.N.dw" counts as "model.N.pw")."""
    if layer.endswith(".dw"):
        layer = layer[:-3] + ".pw"
    return [f for f in ALL_EXACT if f["nref"] == nref and layer in f["layers"]]


_SEL, _FRAME, _DENSE, _BASE = {}, {}, {}, {}


def selector(nref=1):
    if nref not in _SEL:
        _SEL[nref] = selector_state_dict(nref, seed=1)
    return _SEL[nref]


def frame_of(shape):
    if shape not in _FRAME:
        _FRAME[shape] = frame(shape)
    return _FRAME[shape]


def dense_sd(fx):
    if fx["name"] not in _DENSE and fx.get("f16ovf"):
        _DENSE[fx["name"]] = f16ovf_state_dict(selector(fx["nref"]), fx["f16ovf"])
    if fx["name"] not in _DENSE and fx.get("f16sub"):
        _DENSE[fx["name"]] = f16sub_state_dict(selector(fx["nref"]), fx["f16sub"])
    if fx["name"] not in _DENSE and fx.get("elu"):
        _DENSE[fx["name"]] = elu_state_dict(selector(fx["nref"]), fx["j"], fx["elu"])
    if fx["name"] not in _DENSE:
        _DENSE[fx["name"]] = with_dense(selector(fx["nref"]), fx["convs"], seed=fx["seed"], opts=fx["opts"])
    return _DENSE[fx["name"]]


def selector_run(shape, dtype, nref=1, rounding="rne"):
    """The selector network's own reference (with the exactness records), computed once per (frame, dtype, nref, rounding)."""
    key = (shape, dtype, nref, rounding)
    if key not in _BASE:
        r16 = None if rounding == "rne" or dtype == "fp32" else TRUNCATE[dtype]
        _BASE[key] = as_base(selector(nref), reference(selector(nref), frame_of(shape), nref, dtype, round16=r16, probe=True))
    return _BASE[key]


def last_layer(fx):
    return fx["layers"][-1]


def fixture_reference(fx, shape, dtype, sd=None, rounding="rne", probe=False):
    """reference() of a fixture up to its last layer under test, reusing the selector network's layers in front of it."""
    r16 = None if rounding == "rne" or dtype == "fp32" else TRUNCATE[dtype]
    stop = last_layer(fx)
    return reference(sd if sd is not None else dense_sd(fx), frame_of(shape), fx["nref"], dtype,
                     base=selector_run(shape, dtype, fx["nref"], rounding), round16=r16, stop_after=stop, probe=probe)


def exactness(sd, x, nref, dtype, layer, base=None):
    """Headroom and stored range of a fixture whose last layer under test is engine layer ``layer``.

    Returns dict(headroom = the smallest 24 - log2(max sum|t| / q) over every reduction up to ``layer`` (the selectors in front
    of it included), per_reduction = {name: bits}, elu_min = the smallest ELU operand met (must be >= 0), stored_min /
    stored_max = the extreme non-zero magnitudes at the rounding points)."""
    res = reference(sd, x, nref, dtype, base=base, stop_after=layer, probe=True)
    ex = res["_exact"]
    bits = {k: v for k, v in ex.items() if not k.endswith("/elu_min")}
    elu = [v for k, v in ex.items() if k.endswith("/elu_min")]
    st = list(res["_stored"].values())
    return dict(headroom=min(bits.values()), per_reduction=bits, elu_min=min(elu) if elu else 0.0,
                stored_min=min(s[0] for s in st), stored_max=max(s[1] for s in st))


def fixture_exactness(fx, shape, dtype):
    e = exactness(dense_sd(fx), frame_of(shape), fx["nref"], dtype, last_layer(fx), base=selector_run(shape, dtype, fx["nref"]))
    own = [r for c in fx["convs"] for r in reductions_of(c)]
    e["own"] = min(e["per_reduction"][r] for r in own)
    return e


def tap_of(name, taps):
    """float64 oracle activation (oracle.net_ref tap names) that engine layer ``name`` writes: tests/test_kernel_variants.py's."""
    if name.startswith("model.") and name.endswith(".pw"):
        return taps[name[:-3]]
    if name == "cpm.conv":
        return taps["cpm"]
    if name.startswith("cpm.trunk.") and name.endswith(".pw"):
        return taps["cpm.sum"] if name == "cpm.trunk.2.pw" else taps[name[:-3]]
    if name.endswith(".heads.0") or name.endswith(".heads.1"):
        p, k = name[:-len(".heads.0")], name[-1]
        return np.concatenate([taps[p + ".heatmaps." + k], taps[p + ".pafs." + k]], axis=1)
    if name.startswith("refinement_stages.") and name.endswith(".trunk.1") and name.count(".trunk.") == 2:
        return taps[name[:-len(".trunk.1")]]
    return taps[name]


# ------------------------------------------------------------------------------------------------------------ ELU below zero
# Bounded, not exact: the operand z of one ELU of the cpm trunk is exactly known in f32 (a single product of an input k 2^-8
# with a weight -2^e, no bias), negative, and swept from -2^-22 (.pw) or -2^-30 (.dw) down to about -132; the reference is
# expm1(z) in float64 (``reference`` through F.elu).  Everything else is the selector network, so the positive elements of
# the same tensors (one channel in every cycle keeps its weight +1) and every z = 0 stay bit exact.
#
#   fp32         |got - E| <= 1e-6 |E|: Taylor truncation 2.5e-7 at -0.5 plus at most nine roundings of 2^-24 is 7.9e-7; below
#                -0.5 |E| >= 0.39 and the error is at most 2 ulp of exp.  Behind a residual add: + half an f32 ulp of the sum.
#   bf16 / fp16  |got - r16(E)| <= step16(E) + 2^-22: the step (the format's spacing at |E|, the subnormal spacing below the
#                smallest normal) covers the two half-step roundings of the device and of the reference; 2^-22 covers __expf near 1
#                (<= 2 ulp of 2^-24) and a subtraction that is exact or off by half an ulp.  Behind a residual add the stored
#                sum is rounded once more: the step is taken at |E + a|, and where E was rounded before the add (the .dw
#                fixtures: the depthwise result is an MFMA operand) both steps count.
#                Below |z| of about 2^-22 this bound says NOTHING about the 16-bit ELU: exp(z) - 1 in f32 cancels there (at
#                z = -2.9e-8 the bf16 result is 248 bf16 steps off, absolutely 3e-8), and 2^-22 is larger than |E| itself.
#                The .dw fixtures reach that region (they have to: their fp32 form is held to 1e-6 relative down to 2^-30).
ELU_PW_EXP = tuple(range(-14, 7))        # cpm.trunk.J.2 is a packed GEMM weight: 2^-14 is the smallest normal fp16 (exact in bf16)
ELU_DW_EXP = tuple(range(-22, 7))        # depthwise weights stay f32 on every path
ELU_F32_REL = 1e-6
ELU_16_ABS = 2.0 ** -22


def _elu_scale(x, exps, ends=6):
    """Per channel of the tensor ``x`` (N, C, H, W; multiples of 2^-8) the conv under test reads: -2^e, or +1 for the bit-exact
    positive elements.  The ``ends`` channels with the largest values take the largest exponent (one channel in 128 carries
    values up to 531 / 256, a dozen reach 1: only there does |z| pass 2^6 and 104) and the ``ends`` channels with the most
    distinct small odd multiples k 2^-8 (k < 16) the smallest (the lowest binades hold few grid points: all of them are wanted);
    the others cycle through the exponents in between and +1."""
    k = np.rint(x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1) * 256).astype(np.int64)
    n = k.shape[0]
    sc = np.zeros(n)
    top = np.argsort(-k.max(axis=1), kind="stable")[:ends]
    sc[top] = -2.0 ** exps[-1]
    odd = np.array([len({int(v) for v in row if v < 16 and v % 2 == 1}) for row in k], np.int64)
    odd[top] = -1
    low = np.argsort(-odd, kind="stable")[:ends]
    sc[low] = -2.0 ** exps[0]
    rest = np.flatnonzero(sc == 0)
    mid = np.asarray([-2.0 ** e for e in exps[1:-1]] + [1.0])
    sc[rest] = mid[np.arange(rest.size) % mid.size]
    return sc


def elu_state_dict(sd, j, kind):
    """The selector network with the ELU operand of cpm.trunk.J's pointwise ("pw") or depthwise ("dw") conv swept below zero.

    "pw": row o of cpm.trunk.J.2 keeps its one (permuted) input channel with weight -2^e(o).  "dw": the tap of channel c of
    cpm.trunk.J.0 becomes -2^e(c), and cpm.trunk.J.2 copies a negative channel with weight -1: the fused layer then stores
    -(the 16-bit ELU value) >= 0, which the second ELU passes unchanged.  Which channel takes which exponent follows the
    selector network's fp32 activations on the batch-1 frame (the first image of the batch-2 frame), see ``_elu_scale``."""
    out = OrderedDict(sd)
    dwk, pwk = "cpm.trunk.%d.0.weight" % j, "cpm.trunk.%d.2.weight" % j
    acts = selector_run(FRAMES[1], "fp32")[1]
    wp = sd[pwk].numpy().astype(np.float64).reshape(128, 128)
    pick = np.abs(wp).argmax(axis=1)
    if kind == "pw":
        wp = wp * _elu_scale(acts["cpm.trunk.%d.dw" % j].numpy()[:, pick], ELU_PW_EXP)[:, None]
    else:
        sc = _elu_scale(acts["cpm.align" if j == 0 else "cpm.trunk.%d.pw" % (j - 1)].numpy(), ELU_DW_EXP)
        wd = sd[dwk].numpy().astype(np.float64).reshape(128, 9) * sc[:, None]
        out[dwk] = torch.from_numpy(wd.astype(np.float32).reshape(tuple(sd[dwk].shape)))
        wp = wp * np.where(sc[pick] < 0, -1.0, 1.0)[:, None]
    out[pwk] = torch.from_numpy(wp.astype(np.float32).reshape(tuple(sd[pwk].shape)))
    return out


def build_elu_fixtures():
    fx = []
    for j in range(3):
        for kind, conv in (("pw", "cpm.trunk.%d.2" % j), ("dw", "cpm.trunk.%d.0" % j)):
            f = _fixture("elu:cpm.trunk.%d.%s" % (j, kind), [conv])
            f.update(elu=kind, j=j)
            fx.append(f)
    return fx


ELU_FIXTURES = build_elu_fixtures()          # kept apart from FIXTURES: those are compared bit for bit on every element


def elu_fixtures_for(layer):
    """ELU fixtures that engine layer ``layer`` ("cpm.trunk.J.pw", or "cpm.trunk.J.dw" of the unfused graph) runs."""
    return [f for f in ELU_FIXTURES if f["layers"][0][:-3] == layer[:-3]]


def step16(dtype, a):
    """Spacing of the 16-bit format at |a| (the subnormal spacing below its smallest normal number)."""
    mant, emin = (7, -126) if dtype == "bf16" else (10, -14)
    e = np.frexp(np.maximum(np.abs(a), 2.0 ** emin))[1] - 1
    return np.exp2((np.maximum(e, emin) - mant).astype(np.float64))


def _ulp32(a):
    return np.exp2((np.maximum(np.frexp(np.maximum(np.abs(a), 2.0 ** -126))[1] - 1, -126) - 23).astype(np.float64))


def elu_reference(fx, shape, dtype):
    """fixture_reference with the ELU operands recorded (``["_z"]``)."""
    return fixture_reference(fx, shape, dtype, probe=True)


def elu_expect(fx, ref, layer, dtype):
    """What engine layer ``layer`` must hold on an ELU fixture: dict(want = the float64 reference of the stored tensor, bound =
    the allowed |got - want| per element (0: bit exact), neg = the elements behind a negative ELU operand, z = that operand,
    lo / hi = the interval the stored value of a ``neg`` element lies in because the ELU value is in [-1, 0])."""
    j, kind = fx["j"], fx["elu"]
    n_dw, n_pw = "cpm.trunk.%d.dw" % j, "cpm.trunk.%d.pw" % j
    assert layer in (n_dw, n_pw), layer
    want = ref[layer]
    if kind == "pw" and layer == n_dw:                   # the selector depthwise in front of it: operands >= 0, identity
        zero = np.zeros_like(want)
        return dict(want=want, bound=zero, neg=zero.astype(bool), z=ref["_z"][n_dw].numpy(), lo=zero, hi=zero)
    z = ref["_z"][n_pw if kind == "pw" else n_dw].numpy()
    sign = 1.0
    if kind == "dw" and layer == n_pw:                   # read through the +-1 selector behind it
        w2 = dense_sd(fx)["cpm.trunk.%d.2.weight" % j].numpy().astype(np.float64).reshape(128, 128)
        pick = np.abs(w2).argmax(axis=1)
        z = z[:, pick]
        sign = w2[np.arange(128), pick].reshape(1, 128, 1, 1)
    neg = z < 0
    e = np.where(neg, np.expm1(np.minimum(z, 0.0)), z)
    res = layer == n_pw and j == 2
    a = ref["cpm.align"] if res else np.zeros_like(z)
    s = sign * e + a
    if dtype == "fp32":
        bound = ELU_F32_REL * np.abs(e) + (0.5 * _ulp32(s) if res else 0.0)
    else:
        bound = step16(dtype, e) + ELU_16_ABS
        if res:
            bound = step16(dtype, s) + ELU_16_ABS + (step16(dtype, e) if kind == "dw" else 0.0)
    r = ROUND[dtype]
    ends = [r(torch.from_numpy(np.ascontiguousarray(sign * v + a))).numpy() for v in (-1.0, 0.0)]
    return dict(want=want, bound=np.where(neg, bound, 0.0), neg=neg, z=z, lo=np.minimum(*ends), hi=np.maximum(*ends))


def elu_compare(got, exp):
    """(problems, worst error / bound over the elements behind a negative operand) of a device tensor against ``elu_expect``."""
    g = got.astype(np.float64)
    err = np.abs(g - exp["want"])
    neg = exp["neg"]
    bad = []
    exact = ~neg & (g != exp["want"])                     # z = 0 gives 0, positive elements bit for bit (a NaN differs)
    if exact.any():
        bad.append("%d of %d identity / zero elements differ" % (int(exact.sum()), int((~neg).sum())))
    over = neg & ~(err <= exp["bound"])
    if over.any():
        at = tuple(int(v) for v in np.argwhere(over)[0])
        bad.append("%d of %d beyond the bound; first at %s: z %.9g got %.9g want %.9g bound %.3g" % (
            int(over.sum()), int(neg.sum()), at, exp["z"][at], g[at], exp["want"][at], exp["bound"][at]))
    out = neg & ~((g >= exp["lo"]) & (g <= exp["hi"]))
    if out.any():
        at = tuple(int(v) for v in np.argwhere(out)[0])
        bad.append("%d elements outside the image of [-1, 0]; first at %s: got %.9g" % (int(out.sum()), at, g[at]))
    ratio = float((err[neg] / exp["bound"][neg]).max()) if neg.any() else 0.0
    return bad, ratio


# the two device forms restated in float32 NumPy (no fma; exp correctly rounded), and the faults the bounds must bite on
_ELU_COEF = (1.0, 0.5, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040)


def elu_f32_form(z, coef=_ELU_COEF, switch=-0.5):
    """net_kernels.hip's elu_negative on float32 operands <= 0: the degree-7 polynomial above ``switch``, exp - 1 below."""
    v = np.asarray(z, np.float32)
    c = [np.float32(x) for x in coef]
    p = c[6]
    for k in range(5, -1, -1):
        p = (c[k] + (v * p).astype(np.float32)).astype(np.float32)
    p = (v * p).astype(np.float32)
    return np.where(v > np.float32(switch), p, elu_cancelling_form(v))


def elu_cancelling_form(z):
    """The 16-bit paths' __expf(v) - 1 in float32 (before the 16-bit store)."""
    v = np.asarray(z, np.float32)
    return (np.exp(v.astype(np.float64)).astype(np.float32) - np.float32(1)).astype(np.float32)


ELU_MUTANTS = {
    "1/720 in place of 1/5040": lambda z: elu_f32_form(z, coef=_ELU_COEF[:6] + (1.0 / 720,)),
    "switch point at -5": lambda z: elu_f32_form(z, switch=-5.0),
    "the cancelling form at fp32": elu_cancelling_form,
}
