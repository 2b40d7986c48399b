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

Not covered here (they stay with the tolerance tests): ELU's negative branch (a polynomial / the hardware exponential: not
exact; the cpm trunk fixtures keep every ELU operand >= 0, which ``exactness`` checks), fp16 subnormals and overflow, and
the dw<px=2> kernel, which only a 720 x 1280 frame reaches.
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
    a = a[a != 0]
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
    "_stored" per rounding point (smallest, largest non-zero stored magnitude)."""
    h16 = dtype != "fp32"
    r16 = round16 or ROUND[dtype]
    taps, exact, stored = OrderedDict(), OrderedDict(), OrderedDict()
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
            s = float(F.conv2d(xin.abs(), w.abs(), b.abs(), stride, pad, dil, groups).max())
            q = min(_lowbit(xin) * _lowbit(w), _lowbit(b))
            exact[name] = 24.0 - float(np.log2(s / q)) if s > 0 and np.isfinite(q) else 24.0
        return y

    def add(name, a, b):                                  # f32 residual add in an epilogue
        if probe:
            s, q = float((a.abs() + b.abs()).max()), min(_lowbit(a), _lowbit(b))
            exact[name] = 24.0 - float(np.log2(s / q)) if s > 0 and np.isfinite(q) else 24.0
        return a + b

    def elu(name, t):
        if probe:
            exact[name + "/elu_min"] = float(t.min())
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
            for src, dst in ((base[1].get("_exact", {}), exact), (base[1].get("_stored", {}), stored)):
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
        res["_exact"], res["_stored"] = exact, stored
    return res


class _Result(OrderedDict):
    """reference()'s result; ``base`` reuse reads the tensors back through item access."""
    tensors = None


def as_base(sd, res):
    """(sd, {name: tensor}) for ``reference(base=...)``."""
    d = dict(res.tensors)
    for k in ("_exact", "_stored"):
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


FIXTURES = build_fixtures()
BY_NAME = {f["name"]: f for f in FIXTURES}


def fixtures_for(layer, nref=1):
    """Fixtures whose layers under test include engine layer ``layer`` ("model.N.dw" counts as "model.N.pw")."""
    if layer.endswith(".dw"):
        layer = layer[:-3] + ".pw"
    return [f for f in FIXTURES if f["nref"] == nref and layer in f["layers"]]


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
