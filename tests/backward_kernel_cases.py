"""Loop statements, shapes and fixtures for the backward kernels run alone (csrc/bwd_kernels.hip: dgrad, wgrad, wgrad_reduce,
loss_grad, relu_mask, grad_add, elu_grad, dw_dgrad, dw_wgrad, dw_wgrad_reduce, pw_fold, bn_chain).  No GPU in here.

Statements are float64 (or int64: they keep the dtype they are given) and vectorised over channels only: per tap, shifted
slices plus a matmul.  Tensors are NCHW, weights OIHW.  Each statement has an ``abs=True`` form returning sum|terms|, the
quantity the per-element bound is relative to.

Integer fixtures: |dz|, |w|, |x| <= 8 and pre-filled results <= 64 in magnitude, so that every product and every partial sum
is an integer below 2^24 and any summation order, MFMA shape or split count must give the int64 result bit for bit.
Normal fixtures: torch.randn values with exact zeros and one channel of each tensor scaled by 2^-20, so that a per-element
bound bites where a max-norm would not.

The bound of a float32 sum of ``depth`` products, one rounding per operation in any order:
|got - want64| <= (depth + 8) 2^-24 sum|terms|."""
import functools

import numpy as np
import torch

import backbone_backward_cases as bb
import backward_cases as bc

U = 2.0 ** -24
EXACT_LIMIT = 2 ** 24
SMALL = 2.0 ** -20
SENTINEL = -12345.5          # finite, exactly representable, outside every fixture's range of results

# ---------------------------------------------------------------------------------------------- shapes
# dense conv: (N, H, W, cout, cin, ks, dil, pad mode); the 64 x 64 output tile, the 16-deep stage and the pixel ranges
DENSE_SHAPES = [
    (1, 1, 1, 19, 4, 1, 1, "graph"),        # M = 1
    (1, 7, 9, 19, 32, 1, 1, "graph"),       # M = 63
    (2, 8, 4, 38, 68, 3, 1, "graph"),       # M = 64 exactly; 2 frames; a second cin tile 4 wide
    (1, 5, 13, 70, 36, 3, 2, "graph"),      # M = 65; cout crosses a tile and is no multiple of 16; dilation 2
    (3, 2, 3, 57, 132, 3, 2, "graph"),      # map smaller than the dilated kernel; three cin tiles; frames inside one tile
    (1, 12, 11, 128, 185, 1, 1, "graph"),   # the C = 128 concat width
    (2, 3, 5, 32, 36, 1, 1, "raw"),         # pad mode "raw" (cout_pad = cout, cin_pad = cin)
]
# windows of the merged heads: (row stride - channels, channel offset) of dz, x, dx
WINDOWS = ((7, 3), (5, 1), (9, 4))
# the cpm's depthwise 3x3: (N, C, H, W)
DW_SHAPES = [
    (1, 4, 1, 1),        # one pixel, one quad
    (1, 64, 3, 5),       # M = 15: one pixel short of a range; a full channel group
    (2, 68, 2, 4),       # M = 16 exactly; a ragged second channel group; 2 frames
    (1, 132, 1, 17),     # M = 17; three channel groups, the last ragged; a one-row map
    (3, 8, 2, 3),        # frames inside one range
]
# the depthwise 3x3 at stride 1 | 2, dilation 1 | 2 (the backbone's forms), ranges of 16 output pixels: (N, C, H, W)
DW_SD_SHAPES = [
    (2, 8, 5, 7),        # an odd map; 2 frames, their boundary inside a range
    (1, 68, 9, 6),       # an even width; a ragged second channel group
    (1, 4, 2, 3),        # a map smaller than the dilated kernel; a single range
    (3, 4, 8, 8),        # an even map; 3 frames, 12 ranges (3 at stride 2)
]
DW_SD_PAIRS = [(1, 1), (2, 1), (1, 2), (2, 2)]      # (stride, dilation)
# the second trip of the capped grid-stride loops: the smallest size past each cap
CAP_8192 = 8192 * 256        # relu_mask, grad_add, elu_grad (quads), dw_dgrad (quads): threads of the capped grid
CAP_4096 = 4096 * 256        # loss_grad, wgrad_reduce, pw_fold
TRIP_ROWS = (32769, 65)                                  # relu_mask, grad_add: M x C = 2 129 985 elements
TRIP_QUADS = (1, 4, 1025, 2047)                          # elu_grad, dw_dgrad: (N, C, H, W), 2 098 175 quads
TRIP_LOSS = dict(N=2, CH=19, CP=38, h=120, w=120)        # loss_grad: N CP hw = 1 094 400, S = 2
TRIP_REDUCE = (1, 4, 4, 512, 256, 3, 1, "graph")         # wgrad_reduce: 512 x 256 x 9 = 1 179 648 weights, M = 16
TRIP_FOLD = (1024, 1025)                                 # pw_fold: cout x cin = 1 049 600
BN_SHAPES = [(cout, K) for K in (9, 27, 300) for cout in (1, 5)]      # K = 300 crosses the 256-thread stride


def acc_from_values(cin):
    """0 (accumulate everywhere), cin (overwrite) and one value inside a tile that is no multiple of 16, where cin allows."""
    inside = [v for v in (89, 21, 3) if v < cin]
    return [0, cin] + inside[:1]


def dense_M(shape):
    return shape[0] * shape[1] * shape[2]


def dense_pads(shape):
    """(cout_pad, cin_pad) of the packed weight the data gradient reads: the fp32 graph's 64 / 32 padding, or none ("raw")."""
    cout, cin, mode = shape[3], shape[4], shape[7]
    return (cout, cin) if mode == "raw" else ((cout + 63) // 64 * 64, (cin + 31) // 32 * 32)


# ---------------------------------------------------------------------------------------------- dense conv statements
def _taps(ks, dil):
    half = ks // 2
    return [(ky, kx, (ky - half) * dil, (kx - half) * dil) for ky in range(ks) for kx in range(ks)]


def _overlap(H, W, oy, ox):
    """Pixels q = (y, x) for which q + (oy, ox) is inside the map, as slices, and the slices of q + (oy, ox)."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def dense_dgrad(dz, w, dil, abs=False):
    """dX[n, ci, q + off(tap)] += sum_o dZ[n, o, q] W[o, ci, tap]: the forward reads X[q + off(tap)] for Y[q], padding dil (ks / 2)."""
    if abs:
        dz, w = np.abs(dz), np.abs(w)
    N, cout, H, W = dz.shape
    cin, ks = w.shape[1], w.shape[2]
    zr = dz.transpose(0, 2, 3, 1)
    dx = np.zeros((N, H, W, cin), dz.dtype)
    for ky, kx, oy, ox in _taps(ks, dil):
        ov = _overlap(H, W, oy, ox)
        if ov is None:
            continue
        (qy, qx), (sy, sx) = ov
        dx[:, sy, sx, :] += zr[:, qy, qx, :] @ w[:, :, ky, kx]
    return dx.transpose(0, 3, 1, 2)


def dense_wgrad(dz, x, ks, dil, abs=False):
    """dW[o, ci, tap] = sum_q dZ[n, o, q] X[n, ci, q + off(tap)]."""
    if abs:
        dz, x = np.abs(dz), np.abs(x)
    N, cout, H, W = dz.shape
    cin = x.shape[1]
    zr, xr = dz.transpose(0, 2, 3, 1), x.transpose(0, 2, 3, 1)
    dw = np.zeros((cout, cin, ks, ks), dz.dtype)
    for ky, kx, oy, ox in _taps(ks, dil):
        ov = _overlap(H, W, oy, ox)
        if ov is None:
            continue
        (qy, qx), (sy, sx) = ov
        dw[:, :, ky, kx] = zr[:, qy, qx, :].reshape(-1, cout).T @ xr[:, sy, sx, :].reshape(-1, cin)
    return dw


def dense_bias(dz, abs=False):
    return (np.abs(dz) if abs else dz).sum(axis=(0, 2, 3))


def dense_results(dz, x, w, dil, dx0, dw0, db0, acc_from, no_bias, accumulate):
    """What lwp_debug_conv_grad leaves in dx, dw, db (the arrays' own dtype) and sum|terms| of each, prior contents included
    where they are added to."""
    ks = w.shape[2]
    ch = (np.arange(x.shape[1]) >= acc_from).reshape(1, -1, 1, 1)
    g, ga = dense_dgrad(dz, w, dil), dense_dgrad(dz, w, dil, abs=True)
    dx, dx_abs = np.where(ch, dx0 + g, g), np.where(ch, np.abs(dx0) + ga, ga)
    dw, dw_abs = dense_wgrad(dz, x, ks, dil), dense_wgrad(dz, x, ks, dil, abs=True)
    db, db_abs = dense_bias(dz), dense_bias(dz, abs=True)
    if accumulate:
        dw, dw_abs, db, db_abs = dw0 + dw, np.abs(dw0) + dw_abs, db0 + db, np.abs(db0) + db_abs
    if no_bias:
        db, db_abs = db0.copy(), np.zeros_like(db_abs)       # untouched: bit-identical
    return dict(dx=dx, dw=dw, db=db), dict(dx=dx_abs, dw=dw_abs, db=db_abs)


def dense_depths(shape, acc_from, accumulate):
    """Products per output element: taps x cout for dgrad (+ 1 where it accumulates), M (+ 1) for wgrad and the bias sum."""
    N, H, W, cout, cin, ks, dil, _ = shape
    dgrad = ks * ks * cout + (1 if acc_from < cin else 0)
    wgrad = N * H * W + (1 if accumulate else 0)
    return dict(dx=dgrad, dw=wgrad, db=wgrad)


# ---------------------------------------------------------------------------------------------- depthwise statements (stride 1, dilation 1)
def dw_dgrad(dz, w, abs=False):
    """dX[n, c, q + off(tap)] += dZ[n, c, q] w[c, tap] (cpm_backward_cases.dw_dgrad_loops, by slices)."""
    if abs:
        dz, w = np.abs(dz), np.abs(w)
    N, C, H, W = dz.shape
    dx = np.zeros_like(dz)
    for ky, kx, oy, ox in _taps(3, 1):
        ov = _overlap(H, W, oy, ox)
        if ov is None:
            continue
        (qy, qx), (sy, sx) = ov
        dx[:, :, sy, sx] += dz[:, :, qy, qx] * w[:, 0, ky, kx].reshape(1, C, 1, 1)
    return dx


def dw_wgrad(dz, x, abs=False):
    """dW[c, tap] = sum_q dZ[n, c, q] X[n, c, q + off(tap)] (cpm_backward_cases.dw_wgrad_loops, by slices)."""
    if abs:
        dz, x = np.abs(dz), np.abs(x)
    N, C, H, W = dz.shape
    dw = np.zeros((C, 1, 3, 3), dz.dtype)
    for ky, kx, oy, ox in _taps(3, 1):
        ov = _overlap(H, W, oy, ox)
        if ov is None:
            continue
        (qy, qx), (sy, sx) = ov
        dw[:, 0, ky, kx] = (dz[:, :, qy, qx] * x[:, :, sy, sx]).sum(axis=(0, 2, 3))
    return dw


def dw_results(dz, x, w, dx0, dw0, beta, accumulate, dgrad=dw_dgrad, wgrad=dw_wgrad):
    """What lwp_debug_dw_grad leaves in dx and dw, and sum|terms| of each.  ``dgrad`` / ``wgrad``: the statements to use (the
    per-pixel loops of cpm_backward_cases take the same arguments without ``abs``)."""
    a = np.abs
    dx, dx_abs = dgrad(dz, w), dgrad(a(dz), a(w))
    dw, dw_abs = wgrad(dz, x), wgrad(a(dz), a(x))
    if beta:
        dx, dx_abs = dx0 + dx, a(dx0) + dx_abs
    if accumulate:
        dw, dw_abs = dw0 + dw, a(dw0) + dw_abs
    return dict(dx=dx, dw=dw), dict(dx=dx_abs, dw=dw_abs)


def dw_depths(shape, beta, accumulate):
    N, C, H, W = shape
    return dict(dx=9 + (1 if beta else 0), dw=N * H * W + (1 if accumulate else 0))


# ---------------------------------------------------------------------------------------------- element-wise statements
def loss_grad(out, target, mask, scale, abs=False):
    """loss_scale (out - target) mask^2 / batch, ``scale`` = loss_scale / batch as the float32 the host passes; out and target
    (N, C, h, w), mask (N, h, w).  The abs form is |out - target| mask^2 scale: the subtraction is one term, rounded once."""
    d = (out - target) * (mask * mask)[:, None] * scale
    return np.abs(d) if abs else d


def relu_mask(g, y, res=None):
    return np.where(y > (0 if res is None else res), g, np.zeros_like(g))


def grad_add(dst, src, beta, abs=False):
    if abs:
        dst, src = np.abs(dst), np.abs(src)
    return dst + src if beta else src.copy()


def elu_factor(y):
    """elu'(z) from the ELU's output y (alpha = 1): 1 for y > 0, else exp(z) = y + 1."""
    return np.where(y > 0, np.ones_like(y), y + 1)


def elu_grad(g, y, abs=False):
    r = g * elu_factor(y)
    return np.abs(r) if abs else r


def fold(w, gamma, var):
    """float(double(w) * (gamma / sqrt(double(var) + 1e-5))), the scale formed first as the packer forms it; w (cout, cin)."""
    scale = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + 1e-5)
    return (np.asarray(w, np.float64) * scale.reshape(-1, 1)).astype(np.float32)


def bn_chain(G, g, W, b, gamma, mean, var, abs=False):
    """(dW, db, dgamma, dbeta) of backward_cases.bn_chain for G, W (cout, K); the abs form is sum|terms| of dgamma alone."""
    cout, K = np.asarray(G).shape
    if abs:
        inv = 1.0 / np.sqrt(np.asarray(var, np.float64) + 1e-5)
        f = lambda v: np.abs(np.asarray(v, np.float64))
        return ((f(W) * f(G)).sum(1) + f(g) * f(np.asarray(b, np.float64) - np.asarray(mean, np.float64))) * inv
    dW, db, dgamma, dbeta = bc.bn_chain(np.asarray(G).reshape(cout, K, 1, 1), g, np.asarray(W).reshape(cout, K, 1, 1), b, gamma, mean, var)
    return dW.reshape(cout, K), db, dgamma, dbeta


# ---------------------------------------------------------------------------------------------- fixtures
def _seed(key):
    s = 0
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def _ints(rs, shape, bound):
    return rs.randint(-bound, bound + 1, size=shape).astype(np.int64)


def _normal(key, shape, small_axis, zeros=0.1):
    """torch.randn values, a tenth of them exact zeros, the last channel along ``small_axis`` scaled by 2^-20."""
    g = torch.Generator().manual_seed(_seed(key))
    t = torch.randn(*shape, generator=g, dtype=torch.float32)
    t[torch.rand(*shape, generator=g) < zeros] = 0.0
    idx = [slice(None)] * len(shape)
    idx[small_axis] = shape[small_axis] - 1
    t[tuple(idx)] *= SMALL
    return t.numpy()


@functools.lru_cache(maxsize=None)
def dense_fixture(shape, kind, bound=8):
    """dict(dz, x, w, dx0, dw0, db0): int64 arrays (kind "int") or float32 ones (kind "normal") of a dense shape."""
    N, H, W, cout, cin, ks, dil, _ = shape
    sizes = dict(dz=(N, cout, H, W), x=(N, cin, H, W), w=(cout, cin, ks, ks), dx0=(N, cin, H, W), dw0=(cout, cin, ks, ks), db0=(cout,))
    if kind == "int":
        rs = np.random.RandomState(_seed(("dense", shape)))
        return dict((k, _ints(rs, s, 64 if k.endswith("0") else bound)) for k, s in sizes.items())
    small = dict(dz=1, x=1, w=1, dx0=1, dw0=0, db0=0)
    return dict((k, _normal(("dense", shape, k), s, small[k])) for k, s in sizes.items())


@functools.lru_cache(maxsize=None)
def dw_fixture(shape, kind, bound=8, x_bound=8):
    """dict(dz, x, w, dx0, dw0) of a depthwise shape (N, C, H, W)."""
    N, C, H, W = shape
    sizes = dict(dz=(N, C, H, W), x=(N, C, H, W), w=(C, 1, 3, 3), dx0=(N, C, H, W), dw0=(C, 1, 3, 3))
    if kind == "int":
        rs = np.random.RandomState(_seed(("dw", shape)))
        return dict((k, _ints(rs, s, 64 if k.endswith("0") else (x_bound if k == "x" else bound))) for k, s in sizes.items())
    small = dict(dz=1, x=1, w=0, dx0=1, dw0=0)
    return dict((k, _normal(("dw", shape, k), s, small[k])) for k, s in sizes.items())


@functools.lru_cache(maxsize=None)
def dw_sd_fixture(shape, s):
    """dict(dz, x, w) of a depthwise shape at stride ``s``: the integer fixture of the shape, its dz cut to the Ho x Wo map."""
    N, C, H, W = shape
    f = dw_fixture(shape, "int")
    return dict(dz=np.ascontiguousarray(f["dz"][:, :, :(H - 1) // s + 1, :(W - 1) // s + 1]), x=f["x"], w=f["w"])


@functools.lru_cache(maxsize=None)
def dw_sd_reference(shape, s, d):
    """(dict(dx, G, g), sum|terms| of each) of dw_sd_fixture by the pixel loops of backbone_backward_cases, int64.  Computed once
    and shared: do not write to the arrays."""
    N, C, H, W = shape
    f = dw_sd_fixture(shape, s)
    a = np.abs
    G, g = bb.dw_sd_wgrad_loops(f["dz"], f["x"], s, d)
    Ga, ga = bb.dw_sd_wgrad_loops(a(f["dz"]), a(f["x"]), s, d)
    return (dict(dx=bb.dw_sd_dgrad_loops(f["dz"], f["w"], H, W, s, d), G=G, g=g),
            dict(dx=bb.dw_sd_dgrad_loops(a(f["dz"]), a(f["w"]), H, W, s, d), G=Ga, g=ga))


@functools.lru_cache(maxsize=None)
def rows_fixture(shape, kind):
    """dict(g, y, res, src) of an (N, C, H, W) shape for relu_mask, grad_add (dst = g) and elu_grad.  y has exact zeros and, in
    the integer kind, values below -1 as well (the ELU factor y + 1 is then a negative integer)."""
    if kind == "int":
        rs = np.random.RandomState(_seed(("rows", shape)))
        return dict((k, _ints(rs, shape, 8)) for k in ("g", "y", "res", "src"))
    f = dict((k, _normal(("rows", shape, k), shape, 1)) for k in ("g", "y", "res", "src"))
    eq = np.arange(f["y"].size).reshape(shape) % 7 == 0
    f["res"] = np.where(eq, f["y"], f["res"])            # y == res exactly: the mask is strict
    return f


@functools.lru_cache(maxsize=None)
def loss_fixture(N, CH, CP, h, w, S, kind):
    """dict(outs, km, pm, mask, scale): S stage tensors alternating CH and CP channels, NCHW targets, a mask of 0, 1 and 1/2
    (mask^2 is then exact) and scale = float32(loss_scale / batch)."""
    key = ("loss", N, CH, CP, h, w, S)
    rs = np.random.RandomState(_seed(key))
    mask = rs.choice(np.array([0.0, 1.0, 1.0, 0.5]), size=(N, h, w))
    if kind == "int":
        outs = [_ints(rs, (N, CP if s & 1 else CH, h, w), 8) for s in range(S)]
        return dict(outs=outs, km=_ints(rs, (N, CH, h, w), 8), pm=_ints(rs, (N, CP, h, w), 8), mask=np.where(mask == 0.5, 2, mask).astype(np.int64),
                    scale=np.float32(4.0))
    outs = [_normal(key + ("o", s), (N, CP if s & 1 else CH, h, w), 1) for s in range(S)]
    return dict(outs=outs, km=_normal(key + ("km",), (N, CH, h, w), 1), pm=_normal(key + ("pm",), (N, CP, h, w), 1), mask=mask.astype(np.float32),
                scale=np.float32(1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def fold_fixture(cout, cin):
    g = torch.Generator().manual_seed(_seed(("fold", cout, cin)))
    w = torch.randn(cout, cin, generator=g).numpy()
    gamma = torch.randn(cout, generator=g).numpy()
    var = (0.5 + 1.5 * torch.rand(cout, generator=g)).numpy()
    var[cout // 2] = 0.0
    return dict(w=w, gamma=gamma, var=var)


@functools.lru_cache(maxsize=None)
def bn_fixture(cout, K):
    """float32 inputs of bn_chain_kernel and pre-filled outputs; var in [0.5, 2] with one var = 0."""
    g = torch.Generator().manual_seed(_seed(("bn", cout, K)))
    r = lambda *s: torch.randn(*s, generator=g).numpy()
    var = (0.5 + 1.5 * torch.rand(cout, generator=g)).numpy()
    var[cout // 2] = 0.0
    return dict(G=r(cout, K), g=r(cout), W=r(cout, K), b=r(cout), gamma=r(cout), mean=r(cout), var=var,
                dW0=r(cout, K), db0=r(cout), dgamma0=r(cout), dbeta0=r(cout))


def as64(f):
    """A fixture's arrays (and lists of arrays) in float64."""
    conv = lambda v: v.astype(np.float64) if isinstance(v, np.ndarray) else ([conv(i) for i in v] if isinstance(v, list) else v)
    return dict((k, conv(v)) for k, v in f.items())


def max_terms(abs_results):
    """max sum|terms| over the results of an integer fixture: below 2^24 every order of summation is exact."""
    return max(float(np.max(v)) for v in abs_results.values())


# ---------------------------------------------------------------------------------------------- comparisons
def exact_failures(got, want):
    """Names of the results that are not the integer reference on every element (``got`` float32 arrays, ``want`` int64)."""
    bad = []
    for k in want:
        w = np.asarray(want[k])
        assert np.abs(w).max(initial=0) < EXACT_LIMIT, k
        g = torch.from_numpy(np.ascontiguousarray(np.asarray(got[k], np.float32)))
        if g.shape != w.shape or not torch.equal(g, torch.from_numpy(np.ascontiguousarray(w.astype(np.float32)))):
            bad.append(k)
    return bad


def bound_ratios(got, want, terms, depths):
    """Per result, the worst |got - want64| / ((depth + 8) 2^-24 sum|terms|) over the elements; an element whose bound is 0 must
    be exact (infinite ratio otherwise).  A result passes at a ratio <= 1."""
    out = {}
    for k in want:
        err = np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64))
        bnd = (depths[k] + 8) * U * np.asarray(terms[k], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
        out[k] = float(np.max(r)) if r.size else 0.0
    return out


def bound_failures(got, want, terms, depths):
    return [k for k, r in bound_ratios(got, want, terms, depths).items() if not r <= 1.0]


def rounding_ratio(got, want, roundings):
    """Element-wise kernels: worst |got - want64| / (roundings 2^-24 |want64| (1 + 2^-23)) (each rounding is relative to a
    value within a factor 1 + 2^-24 of the result's magnitude; 0 must be exact)."""
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    bnd = roundings * U * np.abs(want) * (1 + 2 * U)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if r.size else 0.0
