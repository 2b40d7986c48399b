"""The backward kernels alone on the GPU (-m gpu): lwp_debug_conv_grad, lwp_debug_dw_grad and the element-wise entry points on the
crafted tensors of tests/backward_kernel_cases.py, at the edges of the 64 x 64 tile, the 16-deep stage, the pixel ranges, the
windows and the capped grid-stride loops.

Integer fixtures: every element equals the int64 statement (torch.equal), whatever the split count.
Normal fixtures, per element: |got - want64| <= (depth + 8) 2^-24 sum|terms|, depth = taps x cout for dgrad (+ 1 where it
accumulates), M (+ 1 with accumulate) for wgrad, bias and the depthwise weight gradient, 9 for the depthwise dgrad: one rounding
per operation in any order.  Element-wise kernels: the roundings of their own formula (<= 2).  pw_fold and bn_chain's dW, db,
dbeta: the float64 statement rounded once (+ one float32 add with accumulate); dgamma: 1 float32 ulp plus (K + 8) 2^-53
sum|terms|, the in-kernel tree adds float64 in another order.  The worst error / bound of each kernel is printed (-s).
Nothing outside a window moves, every call twice gives the same bits, broken argument rules are refused with LWP_ERR_ARG."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine

import backward_kernel_cases as kc
import cpm_backward_cases as cc

pytestmark = pytest.mark.gpu
S = kc.SENTINEL
_eng = []
ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


def engine():
    if not _eng:
        _eng.append(Engine(0, nref=1))
    return _eng[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def twice(call):
    """The call's outputs, after a second identical call gave the same bits."""
    a, b = call(), call()
    for u, v in zip(a, b):
        if torch.is_tensor(u):
            assert torch.equal(u, v)
        else:
            assert u == v
    return a


def untouched(rows, M, lo, hi):
    """The rows behind pixel M and the columns outside [lo, hi) still hold the sentinel, bit for bit."""
    r = host(rows)
    return bool((r[M:] == S).all() and (r[:M, :lo] == S).all() and (r[:M, hi:] == S).all()) and r.shape[0] == M + Engine.GUARD_ROWS


def report(name, ratios):
    print("%s: worst error / bound %s" % (name, ", ".join("%s %.3g" % (k, v) for k, v in sorted(ratios.items()))))


# ---------------------------------------------------------------------------------------------- dense conv: dgrad, wgrad, reduce
def run_dense(shape, f, chunk, acc_from, no_bias, accumulate, windows=None):
    N, H, W, cout, cin, ks, dil, mode = shape
    t = dict((k, dev(v)) for k, v in f.items())
    dx, dw, db, splits, rows = twice(lambda: engine().debug_conv_grad(
        t["dz"], t["x"], t["w"], dil=dil, pad=mode, max_chunk=chunk, acc_from=acc_from, no_bias=no_bias, accumulate=accumulate,
        dx0=t["dx0"], dw0=t["dw0"], db0=t["db0"], windows=windows, fill=S))
    M = kc.dense_M(shape)
    if chunk:
        assert splits == (M + chunk - 1) // chunk
    else:
        assert 1 <= splits <= (M + 63) // 64
    lo = windows[2][1] if windows else 0
    assert untouched(rows, M, lo, lo + cin), (shape, chunk, acc_from, no_bias, accumulate)
    return dict(dx=host(dx), dw=host(dw), db=host(db))


def dense_flags(shape):
    return [(a, nb, acc) for a in kc.acc_from_values(shape[4]) for nb in (0, 1) for acc in (0, 1)]


def windows_of(shape):
    cout, cin = shape[3], shape[4]
    (zp, zo), (xp, xo), (dp, do) = kc.WINDOWS
    return ((cout + zp, zo), (cin + xp, xo), (cin + dp, do))


@pytest.mark.parametrize("shape", kc.DENSE_SHAPES, ids=ids(kc.DENSE_SHAPES))
def test_dense_integer_fixtures_bit_for_bit(shape):
    f = kc.dense_fixture(shape, "int")
    for a, nb, acc in dense_flags(shape):
        want, _ = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, nb, acc)
        for chunk in (0, 16):
            got = run_dense(shape, f, chunk, a, nb, acc)
            assert kc.exact_failures(got, want) == [], (shape, chunk, a, nb, acc)
    a = kc.acc_from_values(shape[4])[-1]
    want, _ = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, 0, 1)
    for chunk in (0, 16):
        assert kc.exact_failures(run_dense(shape, f, chunk, a, 0, 1, windows_of(shape)), want) == [], (shape, chunk, "windows")


@pytest.mark.parametrize("shape", kc.DENSE_SHAPES, ids=ids(kc.DENSE_SHAPES))
def test_dense_normal_fixtures_per_element(shape):
    f32 = kc.dense_fixture(shape, "normal")
    f = kc.as64(f32)
    worst = dict(dx=0.0, dw=0.0, db=0.0)
    cases = [(a, nb, acc, None) for a, nb, acc in dense_flags(shape)] + [(kc.acc_from_values(shape[4])[-1], 0, 1, windows_of(shape))]
    for a, nb, acc, win in cases:
        want, terms = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, nb, acc)
        depths = kc.dense_depths(shape, a, acc)
        for chunk in (0, 16):
            got = run_dense(shape, f32, chunk, a, nb, acc, win)
            r = kc.bound_ratios(got, want, terms, depths)
            worst = dict((k, max(worst[k], r[k])) for k in r)
            assert [k for k in r if not r[k] <= 1.0] == [], (shape, chunk, a, nb, acc, win, r)
    report("dgrad / wgrad + reduce / bias %s" % (shape,), worst)


def test_dense_second_trip_of_the_reduce_kernel():
    """512 x 256 x 9 weights: more than the 4096 x 256 threads of wgrad_reduce's capped grid."""
    shape = kc.TRIP_REDUCE
    f = kc.dense_fixture(shape, "int")
    for acc in (0, 1):
        want, _ = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], shape[4], 0, acc)
        assert kc.exact_failures(run_dense(shape, f, 0, shape[4], 0, acc), want) == []


# ---------------------------------------------------------------------------------------------- the cpm's depthwise 3x3
def run_dw(shape, f, chunk, beta, accumulate, ld=None):
    N, C, H, W = shape
    t = dict((k, dev(v)) for k, v in f.items())
    dx, dw, splits, rows = twice(lambda: engine().debug_cpm_dw_grad(t["dz"], t["x"], t["w"], beta=beta, accumulate=accumulate, max_chunk=chunk,
                                                                    dx0=t["dx0"], dw0=t["dw0"], ld=ld, fill=S))
    M = N * H * W
    if chunk:
        assert splits == (M + chunk - 1) // chunk
    else:
        assert 1 <= splits <= (M + 63) // 64
    assert untouched(rows, M, 0, C), (shape, chunk, beta, accumulate, ld)
    return dict(dx=host(dx), dw=host(dw))


def dw_cases(shape):
    return [(b, a, None) for b in (0, 1) for a in (0, 1)] + [(1, 1, shape[1] + 8)]       # the last one: rows wider than C


@pytest.mark.parametrize("shape", kc.DW_SHAPES, ids=ids(kc.DW_SHAPES))
def test_depthwise_integer_fixtures_bit_for_bit_against_the_pixel_loops(shape):
    f = kc.dw_fixture(shape, "int")
    for beta, acc, ld in dw_cases(shape):
        want, _ = kc.dw_results(f["dz"], f["x"], f["w"], f["dx0"], f["dw0"], beta, acc, cc.dw_dgrad_loops, cc.dw_wgrad_loops)
        for chunk in (0, 16):
            assert kc.exact_failures(run_dw(shape, f, chunk, beta, acc, ld), want) == [], (shape, chunk, beta, acc, ld)


@pytest.mark.parametrize("shape", kc.DW_SHAPES, ids=ids(kc.DW_SHAPES))
def test_depthwise_normal_fixtures_per_element_against_the_pixel_loops(shape):
    f32 = kc.dw_fixture(shape, "normal")
    f = kc.as64(f32)
    worst = dict(dx=0.0, dw=0.0)
    for beta, acc, ld in dw_cases(shape):
        want, terms = kc.dw_results(f["dz"], f["x"], f["w"], f["dx0"], f["dw0"], beta, acc, cc.dw_dgrad_loops, cc.dw_wgrad_loops)
        depths = kc.dw_depths(shape, beta, acc)
        for chunk in (0, 16):
            r = kc.bound_ratios(run_dw(shape, f32, chunk, beta, acc, ld), want, terms, depths)
            worst = dict((k, max(worst[k], r[k])) for k in r)
            assert [k for k in r if not r[k] <= 1.0] == [], (shape, chunk, beta, acc, ld, r)
    report("dw_dgrad / dw_wgrad + reduce %s" % (shape,), worst)


def test_depthwise_second_trip():
    """2 098 175 quads: more than the 8192 x 256 threads of dw_dgrad's capped grid (and 1024 ranges of the weight gradient)."""
    shape = kc.TRIP_QUADS
    f = kc.dw_fixture(shape, "int", 4, 1)
    got = run_dw(shape, f, 0, 1, 1)
    want = dict(dx=f["dx0"] + kc.dw_dgrad(f["dz"], f["w"]), dw=f["dw0"] + kc.dw_wgrad(f["dz"], f["x"]))
    assert kc.exact_failures(got, want) == []


# ---------------------------------------------------------------------------------------------- the same family at stride 1 | 2, dilation 1 | 2
@pytest.mark.parametrize("s,d", kc.DW_SD_PAIRS)
@pytest.mark.parametrize("shape", kc.DW_SD_SHAPES, ids=ids(kc.DW_SD_SHAPES))
def test_strided_depthwise_integer_fixtures_bit_for_bit_against_the_pixel_loops(shape, s, d):
    """lwp_debug_dw_grad_sd (the backbone's form: dz on the Ho x Wo map, the sum of dZ as a tenth row) in ranges of 16 output
    pixels: dx, G and g equal the int64 pixel loops on every element.  At (1, 1) the cpm's entry point returns the same bits on
    the same tensors, integer and normal ones: one kernel family, one order of summation."""
    N, C, H, W = shape
    M = N * ((H - 1) // s + 1) * ((W - 1) // s + 1)
    f = kc.dw_sd_fixture(shape, s)
    want, _ = kc.dw_sd_reference(shape, s, d)
    dz, x, w = dev(f["dz"]), dev(f["x"]), dev(f["w"])
    dx, G, g, splits = twice(lambda: engine().debug_dw_grad(dz, x, w, s, d, max_chunk=16))
    assert splits == (M + 15) // 16
    assert kc.exact_failures(dict(dx=host(dx), G=host(G), g=host(g)), want) == [], (shape, s, d)
    if (s, d) != (1, 1):
        return
    fn = kc.dw_fixture(shape, "normal")
    for dz, x, w in ((dz, x, w), (dev(fn["dz"]), dev(fn["x"]), dev(fn["w"]))):
        dx, G, _, splits = engine().debug_dw_grad(dz, x, w, 1, 1, max_chunk=16)
        dx1, dw1, splits1, _ = engine().debug_cpm_dw_grad(dz, x, w, max_chunk=16)
        assert splits1 == splits and torch.equal(dx1, dx) and torch.equal(dw1, G), shape


# ---------------------------------------------------------------------------------------------- element-wise kernels
ROW_SHAPES = [(2, 8, 3, 5), (1, 68, 1, 7), (1, 4, 1, 1)]
TRIP_ROW_SHAPE = (1, kc.TRIP_ROWS[1], kc.TRIP_ROWS[0], 1)


def rows_results(shape, f, ld):
    """Every element-wise call on a rows fixture: {name: (got, want, roundings)}; windows and rows behind the last pixel checked."""
    N, C, H, W = shape
    t = dict((k, dev(v)) for k, v in f.items())
    e = engine()
    out = {}

    def take(name, call, want, roundings):
        got, rows = twice(call)
        assert untouched(rows, N * H * W, 0, C), (name, shape, ld)
        out[name] = (host(got), want, roundings)
    take("relu_mask", lambda: e.debug_relu_mask(t["g"], t["y"], None, ld, S), kc.relu_mask(f["g"], f["y"]), 0)
    take("relu_mask res", lambda: e.debug_relu_mask(t["g"], t["y"], t["res"], ld, S), kc.relu_mask(f["g"], f["y"], f["res"]), 0)
    take("grad_add 0", lambda: e.debug_grad_add(t["g"], t["src"], 0, ld, S), kc.grad_add(f["g"], f["src"], 0), 0)
    take("grad_add 1", lambda: e.debug_grad_add(t["g"], t["src"], 1, ld, S), kc.grad_add(f["g"], f["src"], 1), 1)
    if C % 4 == 0:
        take("elu_grad", lambda: e.debug_elu_grad(t["g"], t["y"], ld, S), kc.elu_grad(f["g"], f["y"]), 2)
    return out


@pytest.mark.parametrize("shape", ROW_SHAPES + [TRIP_ROW_SHAPE, kc.TRIP_QUADS], ids=ids(ROW_SHAPES + [TRIP_ROW_SHAPE, kc.TRIP_QUADS]))
def test_elementwise_integer_fixtures_bit_for_bit(shape):
    """The last two shapes pass the 8192 x 256 threads of the capped grids: 2 129 985 elements, 2 098 175 quads."""
    f = kc.rows_fixture(shape, "int")
    for ld in (None,) if shape[2] > 100 else (None, shape[1] + 4):
        for name, (got, want, _) in rows_results(shape, f, ld).items():
            assert kc.exact_failures(dict(v=got), dict(v=want)) == [], (name, shape, ld)


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=ids(ROW_SHAPES))
def test_elementwise_normal_fixtures_within_their_own_roundings(shape):
    f32 = kc.rows_fixture(shape, "normal")
    f = kc.as64(f32)
    worst = {}
    for ld in (None, shape[1] + 4):
        for name, (got, want, roundings) in rows_results(shape, f32, ld).items():
            if roundings == 0:
                assert np.array_equal(got.astype(np.float64), want), (name, shape, ld)
                continue
            # the float64 statement on the float32 inputs
            r = kc.rounding_ratio(got, kc.grad_add(f["g"], f["src"], 1) if name == "grad_add 1" else kc.elu_grad(f["g"], f["y"]), roundings)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (name, shape, ld, r)
    report("element-wise %s" % (shape,), worst)


def run_loss(f, ld, off):
    """([gradient per stage tensor], [the statement's]) of a loss fixture; int64 statements for the integer kind."""
    exact = f["km"].dtype == np.int64
    t = f if exact else kc.as64(f)
    n = len(f["outs"])

    def call():
        grads, rows = engine().debug_loss_grad([dev(o) for o in f["outs"]], dev(f["km"]), dev(f["pm"]), dev(f["mask"]), float(f["scale"]), ld, off, S)
        return tuple(grads) + tuple(rows)
    res = twice(call)
    N, CH, h, w = f["km"].shape
    CP = f["pm"].shape[1]
    got, want = [], []
    for s in range(n):
        assert untouched(res[n + s], N * h * w, off, off + (CP if s & 1 else CH)), s
        got.append(host(res[s]))
        want.append(kc.loss_grad(t["outs"][s], t["pm"] if s & 1 else t["km"], t["mask"], int(f["scale"]) if exact else np.float64(f["scale"])))
    return got, want


@pytest.mark.parametrize("dims", [(2, 5, 6, 3, 4, 4), (3, 5, 6, 2, 3, 1), (1, 19, 38, 1, 1, 16), (2, 19, 38, 120, 120, 2)],
                         ids=["small", "one tensor", "16 tensors", "second trip"])
def test_loss_gradient(dims):
    """The last case has N CP hw = 1 094 400 elements: more than the 4096 x 256 threads of loss_grad's capped grid."""
    N, CH, CP, h, w, n = dims
    ld, off = max(CH, CP) + 6, 2
    f = kc.loss_fixture(N, CH, CP, h, w, n, "int")
    got, want = run_loss(f, ld, off)
    for s in range(n):
        assert kc.exact_failures(dict(v=got[s]), dict(v=want[s])) == [], s
    if h * w > 1000:
        return
    got, want = run_loss(kc.loss_fixture(N, CH, CP, h, w, n, "normal"), ld, off)
    worst = max(kc.rounding_ratio(got[s], want[s], 2) for s in range(n))           # the subtraction and the scale; mask^2 is exact
    report("loss_grad %s" % (dims,), dict(grad=worst))
    assert worst <= 1.0


@pytest.mark.parametrize("shape", [(6, 7), (5, 64), kc.TRIP_FOLD], ids=ids([(6, 7), (5, 64), kc.TRIP_FOLD]))
def test_pw_fold_is_the_float64_statement_rounded_once(shape):
    """1024 x 1025 passes the 4096 x 256 threads of the capped grid."""
    f = kc.fold_fixture(*shape)
    got = twice(lambda: (engine().debug_pw_fold(dev(f["w"]), dev(f["gamma"]), dev(f["var"])),))[0]
    want = kc.fold(f["w"], f["gamma"], f["var"])
    assert (f["var"] == 0).sum() == 1 and np.isfinite(want).all()
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("cout,K", kc.BN_SHAPES)
def test_bn_chain_against_the_float64_statement(cout, K):
    f = kc.bn_fixture(cout, K)
    dW, db, dgamma, dbeta = kc.bn_chain(f["G"], f["g"], f["W"], f["b"], f["gamma"], f["mean"], f["var"])
    terms = kc.bn_chain(f["G"], f["g"], f["W"], f["b"], f["gamma"], f["mean"], f["var"], abs=True)
    ins = [dev(f[k]) for k in ("G", "g", "W", "b", "gamma", "mean", "var")]
    worst = 0.0
    for acc in (0, 1):
        for with_db in (1, 0):
            def call():
                # every output sits between two sentinels; dW behind a row of them
                full = dict(dW=torch.full((cout + 2, K), S, device="cuda"), db=torch.full((cout + 2,), S, device="cuda"),
                            dgamma=torch.full((cout + 2,), S, device="cuda"), dbeta=torch.full((cout + 2,), S, device="cuda"))
                for k in full:
                    full[k][1:cout + 1] = dev(f[k + "0"])
                engine().debug_bn_chain(*ins, into=(full["dW"][1:cout + 1], full["db"][1:cout + 1] if with_db else None,
                                                    full["dgamma"][1:cout + 1], full["dbeta"][1:cout + 1]), accumulate=acc)
                torch.cuda.synchronize()
                return tuple(full[k] for k in ("dW", "db", "dgamma", "dbeta"))
            got = dict(zip(("dW", "db", "dgamma", "dbeta"), (host(t) for t in twice(call))))
            for k in got:
                assert (got[k][0] == S).all() and (got[k][-1] == S).all(), (k, acc, with_db)       # the neighbours
            once = lambda v, old: (old + v.astype(np.float32)) if acc else v.astype(np.float32)     # rounded once, then one float32 add
            assert np.array_equal(got["dW"][1:-1], once(dW, f["dW0"])), (acc, with_db)
            assert np.array_equal(got["dbeta"][1:-1], once(dbeta, f["dbeta0"])), (acc, with_db)
            assert np.array_equal(got["db"][1:-1], once(db, f["db0"]) if with_db else f["db0"]), (acc, with_db)
            # dgamma: the float64 tree in another order, one rounding to float32 (within 1 ulp), one more add with accumulate
            want = dgamma + f["dgamma0"].astype(np.float64) if acc else dgamma
            tol = np.spacing(np.abs(dgamma).astype(np.float32)).astype(np.float64) + (K + 8) * 2.0 ** -53 * terms
            if acc:
                tol = tol + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            err = np.abs(got["dgamma"][1:-1].astype(np.float64) - want)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (acc, with_db, err, tol)
    report("bn_chain (%d, %d)" % (cout, K), dict(dgamma=worst))


# ---------------------------------------------------------------------------------------------- argument rules
def test_broken_argument_rules_are_refused_without_a_launch():
    e = engine()
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError, match="raw weights"):
        e.debug_conv_grad(z(1, 19, 2, 2), z(1, 4, 2, 2), z(19, 4, 1, 1), pad="raw")
    with pytest.raises(ValueError, match="max_chunk"):
        e.debug_conv_grad(z(1, 16, 2, 2), z(1, 4, 2, 2), z(16, 4, 1, 1), max_chunk=8)
    with pytest.raises(ValueError, match="ks is 1 or 3"):
        e.debug_conv_grad(z(1, 16, 2, 2), z(1, 4, 2, 2), z(16, 4, 5, 5))
    with pytest.raises(ValueError, match="multiple of 4"):
        e.debug_cpm_dw_grad(z(1, 6, 2, 2), z(1, 6, 2, 2), z(6, 1, 3, 3))
    with pytest.raises(ValueError, match="max_chunk"):
        e.debug_cpm_dw_grad(z(1, 8, 2, 2), z(1, 8, 2, 2), z(8, 1, 3, 3), max_chunk=8)
    with pytest.raises(ValueError, match="multiples of 4"):
        e.debug_elu_grad(z(1, 6, 2, 2), z(1, 6, 2, 2))
    lib = _lib.lib()
    assert lib.lwp_debug_conv_grad(e.h.ptr, None, 4, 0, None, 4, 0, None, 1, 1, 1, 4, 4, 1, 1, 0, 0, 4, 0, 0, None, 4, 0, None, None, None) == _lib.LWP_ERR_ARG
