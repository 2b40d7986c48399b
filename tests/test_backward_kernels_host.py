"""tests/backward_kernel_cases.py checked on the CPU (-m "not gpu"): every loop statement against torch's float64 autograd, the
fold against the packer's, the integer fixtures' exactness condition, the launchers' argument rules on every shape, and the
comparison functions of tests/test_gpu_backward_kernels.py against mutated references: each mutation must be reported, by the
exact comparison and by the bounded one.  (A broken kernel is never run: the mutations are on the reference side.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_cases as bc
import backward_kernel_cases as kc
import cpm_backward_cases as cc
import exact_cases as ec

REL = 1e-12
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


def close(got, want, terms):
    """Per element within 1e-12 of sum|terms| (float64 in another summation order)."""
    return bool((np.abs(got - want) <= REL * np.maximum(terms, np.abs(want))).all())


# ---------------------------------------------------------------------------------------------- statements against autograd
@pytest.mark.parametrize("shape", kc.DENSE_SHAPES, ids=ids(kc.DENSE_SHAPES))
def test_dense_statements_equal_float64_autograd(shape):
    N, H, W, cout, cin, ks, dil, _ = shape
    f = kc.as64(kc.dense_fixture(shape, "normal"))
    x, w, b = T(f["x"]).requires_grad_(), T(f["w"]).requires_grad_(), torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w, b, 1, dil * (ks // 2), dil).backward(T(f["dz"]))
    assert close(kc.dense_dgrad(f["dz"], f["w"], dil), x.grad.numpy(), kc.dense_dgrad(f["dz"], f["w"], dil, abs=True))
    assert close(kc.dense_wgrad(f["dz"], f["x"], ks, dil), w.grad.numpy(), kc.dense_wgrad(f["dz"], f["x"], ks, dil, abs=True))
    assert close(kc.dense_bias(f["dz"]), b.grad.numpy(), kc.dense_bias(f["dz"], abs=True))
    # the integer fixture through the same statements: int64 and float64 agree exactly
    g = kc.dense_fixture(shape, "int")
    g64 = kc.as64(g)
    assert np.array_equal(kc.dense_dgrad(g["dz"], g["w"], dil), kc.dense_dgrad(g64["dz"], g64["w"], dil))
    assert np.array_equal(kc.dense_wgrad(g["dz"], g["x"], ks, dil), kc.dense_wgrad(g64["dz"], g64["x"], ks, dil))


@pytest.mark.parametrize("shape", kc.DW_SHAPES, ids=ids(kc.DW_SHAPES))
def test_depthwise_statements_equal_float64_autograd_and_the_pixel_loops(shape):
    N, C, H, W = shape
    f = kc.as64(kc.dw_fixture(shape, "normal"))
    x, w = T(f["x"]).requires_grad_(), T(f["w"]).requires_grad_()
    F.conv2d(x, w, None, 1, 1, 1, C).backward(T(f["dz"]))
    dx, dw = kc.dw_dgrad(f["dz"], f["w"]), kc.dw_wgrad(f["dz"], f["x"])
    dxa, dwa = kc.dw_dgrad(f["dz"], f["w"], abs=True), kc.dw_wgrad(f["dz"], f["x"], abs=True)
    assert close(dx, x.grad.numpy(), dxa) and close(dw, w.grad.numpy(), dwa)
    assert close(dx, cc.dw_dgrad_loops(f["dz"], f["w"]), dxa) and close(dw, cc.dw_wgrad_loops(f["dz"], f["x"]), dwa)
    g = kc.dw_fixture(shape, "int")
    assert np.array_equal(kc.dw_dgrad(g["dz"], g["w"]), cc.dw_dgrad_loops(g["dz"], g["w"]))
    assert np.array_equal(kc.dw_wgrad(g["dz"], g["x"]), cc.dw_wgrad_loops(g["dz"], g["x"]))


def test_elementwise_statements_equal_float64_autograd():
    shape = (2, 8, 3, 5)
    f = kc.as64(kc.rows_fixture(shape, "normal"))
    # ELU: y = elu(z); the statement reads y only
    z = T(f["y"]).requires_grad_()
    y = F.elu(z)
    y.backward(T(f["g"]))
    want = z.grad.numpy()
    assert np.abs(kc.elu_grad(f["g"], y.detach().numpy()) - want).max() <= REL * np.abs(want).max()
    assert np.array_equal(kc.elu_factor(np.array([-3.0, -1.0, 0.0, 2.0])), np.array([-2.0, 0.0, 1.0, 1.0]))
    # ReLU with a residual behind it: y = relu(z) + res
    z = T(f["y"]).requires_grad_()
    out = F.relu(z) + T(f["res"])
    out.backward(T(f["g"]))
    assert np.array_equal(kc.relu_mask(f["g"], out.detach().numpy(), f["res"]), z.grad.numpy())
    assert np.array_equal(kc.relu_mask(f["g"], F.relu(z).detach().numpy()), z.grad.numpy())
    # masked L2 loss
    lf = kc.as64(kc.loss_fixture(2, 5, 6, 3, 4, 4, "normal"))
    outs = [T(o).requires_grad_() for o in lf["outs"]]
    batch, loss_scale = 3, 0.75
    bc.loss(outs, T(lf["km"]), T(lf["pm"]), T(lf["mask"]), batch, loss_scale).backward()
    for s, o in enumerate(outs):
        got = kc.loss_grad(lf["outs"][s], lf["pm"] if s & 1 else lf["km"], lf["mask"], loss_scale / batch)
        assert np.abs(got - o.grad.numpy()).max() <= REL * np.abs(o.grad.numpy()).max()
    assert set(np.unique(lf["mask"])) == {0.0, 0.5, 1.0}


def test_fold_is_the_packers_and_the_chain_rule_is_backward_cases():
    f = kc.fold_fixture(6, 7)
    sd = {"c.weight": torch.from_numpy(f["w"]).reshape(6, 7, 1, 1), "n.weight": torch.from_numpy(f["gamma"]),
          "n.running_var": torch.from_numpy(f["var"]), "n.running_mean": torch.zeros(6), "n.bias": torch.zeros(6)}
    w, _ = ec.fold(sd, "c", "n")
    got = kc.fold(f["w"], f["gamma"], f["var"])
    assert got.dtype == np.float32 and f["var"][3] == 0.0
    assert np.array_equal(got.astype(np.float64), w.reshape(6, 7).numpy())
    for cout, K in kc.BN_SHAPES:
        b = kc.bn_fixture(cout, K)
        assert (b["var"] == 0).sum() == 1 and ((b["var"] == 0) | ((b["var"] >= 0.5) & (b["var"] <= 2))).all()
        dW, db, dgamma, dbeta = kc.bn_chain(b["G"], b["g"], b["W"], b["b"], b["gamma"], b["mean"], b["var"])
        ref = bc.bn_chain(b["G"].reshape(cout, K, 1, 1), b["g"], b["W"].reshape(cout, K, 1, 1), b["b"], b["gamma"], b["mean"], b["var"])
        assert np.array_equal(dW, ref[0].reshape(cout, K)) and np.array_equal(dgamma, ref[2])
        assert (np.abs(dgamma) <= kc.bn_chain(b["G"], b["g"], b["W"], b["b"], b["gamma"], b["mean"], b["var"], abs=True)).all()


# ---------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("shape", kc.DENSE_SHAPES + [kc.TRIP_REDUCE], ids=ids(kc.DENSE_SHAPES + [kc.TRIP_REDUCE]))
def test_dense_integer_fixtures_are_exact_and_shapes_obey_the_launchers(shape):
    N, H, W, cout, cin, ks, dil, mode = shape
    f = kc.dense_fixture(shape, "int")
    for k, v in f.items():
        assert v.dtype == np.int64 and np.abs(v).max() <= (64 if k.endswith("0") else 8), k
    _, terms = kc.dense_results(f["dz"], f["x"], f["w"], dil, f["dx0"], f["dw0"], f["db0"], 0, 0, 1)      # everything accumulates: the largest sums
    assert kc.max_terms(terms) < kc.EXACT_LIMIT
    # launch_dgrad / launch_wgrad / lwp_debug_conv_grad
    cout_pad, cin_pad = kc.dense_pads(shape)
    assert ks in (1, 3) and dil in (1, 2) and 1 <= cout <= cout_pad and 1 <= cin <= cin_pad and cin_pad % 4 == 0 and cout_pad % 16 == 0
    if mode == "raw":
        assert cout % 16 == 0 and cin % 4 == 0
    assert all(0 <= a <= cin for a in kc.acc_from_values(cin))
    inside = [a for a in kc.acc_from_values(cin) if 0 < a < cin]
    assert all(a % 16 for a in inside) and (inside or cin <= 4)
    assert (kc.dense_M(shape) + 15) // 16 <= 65535


def test_dense_shapes_reach_the_edges_they_name():
    Ms = [kc.dense_M(s) for s in kc.DENSE_SHAPES]
    assert Ms[:4] == [1, 63, 64, 65] and kc.DENSE_SHAPES[2][0] == 2
    assert kc.DENSE_SHAPES[2][4] == 64 + 4 and kc.DENSE_SHAPES[3][3] > 64 and kc.DENSE_SHAPES[3][3] % 16
    N, H, W, cout, cin, ks, dil, _ = kc.DENSE_SHAPES[4]
    assert H <= dil and W <= dil * 2 and cin > 128 and H * W < 64 < N * H * W * 4
    assert kc.DENSE_SHAPES[5][3] == 128 and kc.DENSE_SHAPES[6][7] == "raw"
    assert [s[0] * s[2] * s[3] for s in kc.DW_SHAPES] == [1, 15, 16, 17, 18]
    assert kc.TRIP_ROWS[0] * kc.TRIP_ROWS[1] > kc.CAP_8192 and kc.TRIP_ROWS[1] % 4
    n, c, h, w = kc.TRIP_QUADS
    assert n * h * w * (c // 4) > kc.CAP_8192 and c == 4
    t = kc.TRIP_LOSS
    assert t["N"] * t["CP"] * t["h"] * t["w"] > kc.CAP_4096
    assert kc.TRIP_REDUCE[3] * kc.TRIP_REDUCE[4] * 9 > kc.CAP_4096 and kc.dense_M(kc.TRIP_REDUCE) == 16
    assert kc.TRIP_FOLD[0] * kc.TRIP_FOLD[1] > kc.CAP_4096


@pytest.mark.parametrize("shape", kc.DW_SHAPES, ids=ids(kc.DW_SHAPES))
def test_depthwise_integer_fixtures_are_exact_and_shapes_obey_the_launchers(shape):
    N, C, H, W = shape
    f = kc.dw_fixture(shape, "int")
    _, terms = kc.dw_results(f["dz"], f["x"], f["w"], f["dx0"], f["dw0"], 1, 1)
    assert kc.max_terms(terms) < kc.EXACT_LIMIT
    assert C >= 4 and C % 4 == 0 and (N * H * W + 15) // 16 <= 65535


@pytest.mark.parametrize("s,d", kc.DW_SD_PAIRS)
@pytest.mark.parametrize("shape", kc.DW_SD_SHAPES, ids=ids(kc.DW_SD_SHAPES))
def test_strided_depthwise_integer_fixtures_are_exact_and_the_loops_are_float64_autograd(shape, s, d):
    N, C, H, W = shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    f = kc.dw_sd_fixture(shape, s)
    assert f["dz"].shape == (N, C, Ho, Wo) and f["dz"].dtype == np.int64
    assert max(np.abs(f[k]).max() for k in ("dz", "x", "w")) <= 8
    want, terms = kc.dw_sd_reference(shape, s, d)
    # every sum of |terms| is below 2^24: each partial sum, in any order and any split into ranges, is an exact float32 integer
    assert kc.max_terms(terms) < kc.EXACT_LIMIT
    assert all(v.dtype == np.int64 for v in want.values())
    assert C >= 4 and C % 4 == 0 and (N * Ho * Wo + 15) // 16 <= 65535
    x, w = T(f["x"].astype(np.float64)).requires_grad_(), T(f["w"].astype(np.float64)).requires_grad_()
    F.conv2d(x, w, None, s, d, d, C).backward(T(f["dz"].astype(np.float64)))
    assert np.array_equal(x.grad.numpy(), want["dx"]) and np.array_equal(w.grad.numpy(), want["G"])
    assert np.array_equal(f["dz"].sum(axis=(0, 2, 3)), want["g"])
    if (s, d) == (1, 1):                               # the cpm's statements on the same tensors
        assert np.array_equal(kc.dw_dgrad(f["dz"], f["w"]), want["dx"]) and np.array_equal(kc.dw_wgrad(f["dz"], f["x"]), want["G"])


def test_strided_depthwise_shapes_reach_the_edges_they_name():
    (a, b, c, e), ranges = kc.DW_SD_SHAPES, lambda sh, s: (sh[0] * ((sh[2] - 1) // s + 1) * ((sh[3] - 1) // s + 1) + 15) // 16
    assert a[2] % 2 and a[3] % 2 and a[0] == 2 and (a[2] * a[3]) % 16            # odd map; the frame boundary is inside a range
    assert b[3] % 2 == 0 and 64 < b[1] < 128                                     # even width; a ragged second channel group
    assert c[2] < 3 and c[3] <= 3 and ranges(c, 1) == 1                          # smaller than the kernel at dilation 2 (span 5)
    assert e[2] % 2 == 0 and e[3] % 2 == 0 and (ranges(e, 1), ranges(e, 2)) == (12, 3)
    assert all(ranges(sh, 1) > 1 for sh in (a, b, e)) and all(ranges(sh, 2) > 1 for sh in (a, e))


def test_second_trip_fixtures_are_exact():
    f = kc.dw_fixture(kc.TRIP_QUADS, "int", 4, 1)
    assert np.abs(f["x"]).max() == 1 and np.abs(f["dz"]).max() == 4
    _, terms = kc.dw_results(f["dz"], f["x"], f["w"], f["dx0"], f["dw0"], 1, 1)
    assert kc.max_terms(terms) < kc.EXACT_LIMIT
    t = kc.TRIP_LOSS
    lf = kc.loss_fixture(t["N"], t["CH"], t["CP"], t["h"], t["w"], 2, "int")
    for s, o in enumerate(lf["outs"]):
        assert np.abs(kc.loss_grad(o, lf["pm"] if s & 1 else lf["km"], lf["mask"], int(lf["scale"]))).max() < kc.EXACT_LIMIT


# ---------------------------------------------------------------------------------------------- mutations on the reference side
SHAPE = kc.DENSE_SHAPES[2]         # (2, 8, 4, 38, 68, 3, 1): 3 x 3, two frames, a ragged cin tile
ACC = 21
FILL = 3


def dense_reference(f, acc_from=ACC, no_bias=0, accumulate=1, **swap):
    g = dict(f, **swap)
    return kc.dense_results(g["dz"], g["x"], g["w"], SHAPE[6], g["dx0"], g["dw0"], g["db0"], acc_from, no_bias, accumulate)


def drop_last_pixel(f):
    dz = f["dz"].copy()
    dz[-1, :, -1, -1] = 0
    got, _ = dense_reference(f, dz=dz)
    return dict(dense_reference(f)[0], dw=got["dw"], db=got["db"])


def swap_two_taps(f):
    w = f["w"].copy()
    w[:, :, 0, 1], w[:, :, 2, 1] = f["w"][:, :, 2, 1], f["w"][:, :, 0, 1]
    got = dict(dense_reference(f, w=w)[0])
    true = dense_reference(f)[0]["dw"]
    got["dw"] = true.copy()
    got["dw"][:, :, 0, 1], got["dw"][:, :, 2, 1] = true[:, :, 2, 1], true[:, :, 0, 1]
    return got


def zero_last_input_channel(f):
    x, w = f["x"].copy(), f["w"].copy()
    x[:, -1] = 0
    w[:, -1] = 0
    return dense_reference(f, x=x, w=w)[0]


def overwrite_at_acc_from(f):
    return dense_reference(f, acc_from=ACC + 1)[0]          # channel acc_from itself overwritten: an off-by-one in the comparison


def accumulate_sense_inverted(f):
    got = dict(dense_reference(f)[0])
    g = kc.dense_dgrad(f["dz"], f["w"], SHAPE[6])
    got["dx"] = np.where((np.arange(SHAPE[4]) < ACC).reshape(1, -1, 1, 1), f["dx0"] + g, g)
    return got


def shift_dz_window(f):
    dz = np.concatenate([f["dz"][:, 1:], np.full_like(f["dz"][:, :1], FILL)], axis=1)
    return dense_reference(f, dz=dz)[0]


def shift_dx_window(f):
    got = dict(dense_reference(f)[0])
    got["dx"] = np.concatenate([np.full_like(got["dx"][:, :1], FILL), got["dx"][:, :-1]], axis=1)
    return got


MUTATIONS = [drop_last_pixel, swap_two_taps, zero_last_input_channel, overwrite_at_acc_from, accumulate_sense_inverted, shift_dz_window,
             shift_dx_window]


def as_device(got):
    return dict((k, np.asarray(v, np.float64).astype(np.float32)) for k, v in got.items())


def test_the_unmutated_reference_passes_both_comparisons():
    fi = kc.dense_fixture(SHAPE, "int")
    want, _ = dense_reference(fi)
    assert kc.exact_failures(as_device(want), want) == []
    fn = kc.as64(kc.dense_fixture(SHAPE, "normal"))
    want, terms = dense_reference(fn)
    assert kc.bound_failures(as_device(want), want, terms, kc.dense_depths(SHAPE, ACC, 1)) == []


@pytest.mark.parametrize("mutation", MUTATIONS, ids=[m.__name__ for m in MUTATIONS])
def test_dense_mutations_are_reported_by_both_comparisons(mutation):
    fi = kc.dense_fixture(SHAPE, "int")
    want, _ = dense_reference(fi)
    bad = kc.exact_failures(as_device(mutation(fi)), want)
    assert bad, "the exact comparison misses %s" % mutation.__name__
    fn = kc.as64(kc.dense_fixture(SHAPE, "normal"))
    want, terms = dense_reference(fn)
    bad_n = kc.bound_failures(as_device(mutation(fn)), want, terms, kc.dense_depths(SHAPE, ACC, 1))
    assert bad_n == bad, "the bounded comparison reports %s, the exact one %s" % (bad_n, bad)


DW_SHAPE = kc.DW_SHAPES[2]          # (2, 68, 2, 4)


def dw_reference(f, beta=1, accumulate=1, **swap):
    g = dict(f, **swap)
    return kc.dw_results(g["dz"], g["x"], g["w"], g["dx0"], g["dw0"], beta, accumulate)


def dw_drop_last_pixel(f):
    dz = f["dz"].copy()
    dz[-1, :, -1, -1] = 0
    return dict(dw_reference(f)[0], dw=dw_reference(f, dz=dz)[0]["dw"])


def dw_swap_two_taps(f):
    w = f["w"].copy()
    w[:, 0, 0, 1], w[:, 0, 2, 1] = f["w"][:, 0, 2, 1], f["w"][:, 0, 0, 1]
    got = dict(dw_reference(f, w=w)[0])
    true = dw_reference(f)[0]["dw"]
    got["dw"] = true.copy()
    got["dw"][:, 0, 0, 1], got["dw"][:, 0, 2, 1] = true[:, 0, 2, 1], true[:, 0, 0, 1]
    return got


def dw_zero_last_quad(f):
    """The ragged channel group's only quad left out (the c_in guard one group too early)."""
    x, w = f["x"].copy(), f["w"].copy()
    x[:, -4:] = 0
    w[-4:] = 0
    return dw_reference(f, x=x, w=w)[0]


def dw_overwrite_instead_of_add(f):
    return dw_reference(f, beta=0, accumulate=0)[0]


DW_MUTATIONS = [dw_drop_last_pixel, dw_swap_two_taps, dw_zero_last_quad, dw_overwrite_instead_of_add]


@pytest.mark.parametrize("mutation", DW_MUTATIONS, ids=[m.__name__ for m in DW_MUTATIONS])
def test_depthwise_mutations_are_reported_by_both_comparisons(mutation):
    fi = kc.dw_fixture(DW_SHAPE, "int")
    want, _ = dw_reference(fi)
    assert kc.exact_failures(as_device(want), want) == []
    bad = kc.exact_failures(as_device(mutation(fi)), want)
    assert bad
    fn = kc.as64(kc.dw_fixture(DW_SHAPE, "normal"))
    want, terms = dw_reference(fn)
    depths = kc.dw_depths(DW_SHAPE, 1, 1)
    assert kc.bound_failures(as_device(want), want, terms, depths) == []
    assert kc.bound_failures(as_device(mutation(fn)), want, terms, depths) == bad


def test_elementwise_mutations_are_reported():
    shape = (1, 8, 3, 5)
    fi, fn = kc.rows_fixture(shape, "int"), kc.as64(kc.rows_fixture(shape, "normal"))
    for f, exact in ((fi, True), (fn, False)):
        def differs(got, want, roundings):
            if exact:
                return bool(kc.exact_failures(dict(v=np.asarray(got, np.float64).astype(np.float32)), dict(v=want)))
            return not kc.rounding_ratio(np.asarray(got, np.float64).astype(np.float32), want, roundings) <= 1.0
        want = kc.relu_mask(f["g"], f["y"], f["res"])
        assert not differs(want, want, 1)
        assert differs(np.where(f["y"] >= f["res"], f["g"], 0), want, 1)                  # y == res passes the gradient
        assert differs(kc.relu_mask(f["g"], f["y"]), want, 1)                             # the residual ignored
        want = kc.elu_grad(f["g"], f["y"])
        assert not differs(want, want, 2)
        assert differs(f["g"] * np.where(f["y"] > 0, 1, f["y"]), want, 2)                 # y instead of y + 1
        assert differs(f["g"] * np.where(f["y"] > 0, 1, np.maximum(f["y"], -1) + 1), want, 2)               # clamped at y = -1
        want = kc.grad_add(f["g"], f["src"], 1)
        assert not differs(want, want, 1) and differs(kc.grad_add(f["g"], f["src"], 0), want, 1)
    assert (fi["y"] == 0).any() and (fi["y"] < -1).any() and (fn["y"] == 0).any() and (fn["y"] < -1).any()
    # a second trip that is never taken: everything behind the capped grid left as it was
    M, C = kc.TRIP_ROWS
    f = kc.rows_fixture((1, C, M, 1), "int")
    want = kc.grad_add(f["g"], f["src"], 1)
    flat = np.arange(M * C).reshape(1, M, 1, C).transpose(0, 3, 1, 2)                      # the kernel's index: pixel-major rows
    got = np.where(flat < kc.CAP_8192, want, f["g"])
    assert kc.exact_failures(dict(v=got.astype(np.float32)), dict(v=want)) == ["v"]
    # the loss gradient with the mask not squared
    lf = kc.as64(kc.loss_fixture(2, 5, 6, 3, 4, 2, "normal"))
    want = kc.loss_grad(lf["outs"][1], lf["pm"], lf["mask"], 0.25)
    got = (lf["outs"][1] - lf["pm"]) * lf["mask"][:, None] * 0.25
    assert kc.rounding_ratio(want.astype(np.float32), want, 2) <= 1.0 < kc.rounding_ratio(got.astype(np.float32), want, 2)
