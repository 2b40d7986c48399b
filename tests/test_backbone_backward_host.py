"""CPU: the restatement the backbone-backward tests differentiate (tests/backbone_backward_cases.py) against the oracle's forward
taps, the loop statements of the strided / dilated depthwise gradients, the depthwise bias sum and the stem's weight gradient
against float64 autograd, and the gradient layout and parameter groups of train scope "all" (LWP_TRAIN_ALL)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from oracle import net_ref

import backbone_backward_cases as bb
import backward_cases as bc
import cpm_backward_cases as cc


def case_inputs(name):
    c = bb.CASES[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, sd, x


@pytest.mark.parametrize("name", ["s", "t", "u", "v"])
def test_restatement_equals_the_oracle_taps(name):
    c, sd, x = case_inputs(name)
    taps = {}
    net_ref.forward64(sd, torch.from_numpy(x), c["nref"], taps, stop_after="model.11")
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    acts = {}
    out = bb.backbone(sd64, torch.from_numpy(x).double(), acts=acts)
    assert list(acts) == bb.RELU_LAYERS
    assert tuple(out.shape[2:]) == bb.map_dims(c) and out.shape[1] == 512
    for nm in bb.RELU_LAYERS:
        o = taps[nm]
        assert acts[nm].shape == o.shape, nm
        assert float((acts[nm] - o).abs().max()) <= 1e-12 * max(float(o.max() - o.min()), 1e-300), nm


def test_case_maps_are_the_ones_the_cases_are_chosen_for():
    dims = lambda n: [bb.map_dims(bb.CASES[n], lv) for lv in (1, 2, 3)]
    assert dims("s") == [(18, 22), (9, 11), (5, 6)]
    assert dims("t") == [(15, 10), (8, 5), (4, 3)]
    assert dims("u")[2] == (2, 3)


@pytest.mark.parametrize("s,d", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_depthwise_gradient_formulas_equal_autograd(s, d):
    """Odd and even maps, a map smaller than the dilated kernel (every non-centre tap outside), a 1 x 1 map."""
    g = torch.Generator().manual_seed(31 + 2 * s + d)
    for N, Cn, H, W in ((2, 5, 5, 4), (1, 3, 4, 7), (1, 5, 2, 3), (1, 2, 1, 1), (1, 3, 9, 6)):
        x = torch.randn(N, Cn, H, W, dtype=torch.float64, generator=g).requires_grad_(True)
        w = torch.randn(Cn, 1, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
        b = torch.zeros(Cn, dtype=torch.float64, requires_grad=True)
        z = F.conv2d(x, w, b, s, d, d, Cn)
        assert tuple(z.shape[2:]) == ((H - 1) // s + 1, (W - 1) // s + 1)
        dz = torch.randn(z.shape, dtype=torch.float64, generator=g)
        dx, dw, db = torch.autograd.grad((z * dz).sum(), [x, w, b])
        got_dx = bb.dw_sd_dgrad_loops(dz.numpy(), w.detach().numpy(), H, W, s, d)
        got_dw, got_g = bb.dw_sd_wgrad_loops(dz.numpy(), x.detach().numpy(), s, d)
        assert np.abs(got_dx - dx.numpy()).max() <= 1e-13 * max(1.0, float(dx.abs().max()))
        assert np.abs(got_dw - dw.numpy()).max() <= 1e-13 * max(1.0, float(dw.abs().max()))
        assert np.abs(got_g - db.numpy()).max() <= 1e-13 * max(1.0, float(db.abs().max()))
        if (s, d) == (1, 1):                     # the stride-1 / dilation-1 statements are the cpm's
            assert np.array_equal(got_dx, cc.dw_dgrad_loops(dz.numpy(), w.detach().numpy()))
            assert np.array_equal(got_dw, cc.dw_wgrad_loops(dz.numpy(), x.detach().numpy()))


def test_stem_weight_gradient_formula_equals_autograd():
    g = torch.Generator().manual_seed(41)
    for N, H, W in ((2, 7, 6), (1, 8, 9), (1, 1, 1)):
        x = torch.randn(N, 3, H, W, dtype=torch.float64, generator=g)
        w = torch.randn(32, 3, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
        b = torch.zeros(32, dtype=torch.float64, requires_grad=True)
        z = F.conv2d(x, w, b, 2, 1)
        dz = torch.randn(z.shape, dtype=torch.float64, generator=g)
        dw, db = torch.autograd.grad((z * dz).sum(), [w, b])
        got_dw, got_g = bb.stem_wgrad_loops(dz.numpy(), x.numpy())
        assert np.abs(got_dw - dw.numpy()).max() <= 1e-13 * max(1.0, float(dw.abs().max()))
        assert np.abs(got_g - db.numpy()).max() <= 1e-13 * max(1.0, float(db.abs().max()))


def test_bn_chain_of_a_conv_without_bias_equals_autograd():
    """The chain rule the backbone layers use (backward_cases.bn_chain with b = 0) on a depthwise stride-2 layer."""
    g = torch.Generator().manual_seed(43)
    Cn = 6
    x = torch.randn(2, Cn, 7, 5, dtype=torch.float64, generator=g)
    w = torch.randn(Cn, 1, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
    gamma = (torch.rand(Cn, dtype=torch.float64, generator=g) + 0.5).requires_grad_(True)
    beta = torch.randn(Cn, dtype=torch.float64, generator=g).requires_grad_(True)
    mean = torch.randn(Cn, dtype=torch.float64, generator=g)
    var = torch.rand(Cn, dtype=torch.float64, generator=g) + 0.5
    z = F.batch_norm(F.conv2d(x, w, None, 2, 1, 1, Cn), mean, var, gamma, beta, False, 0.0, 1e-5)
    dz = torch.randn(z.shape, dtype=torch.float64, generator=g)
    dw, dgamma, dbeta = torch.autograd.grad((z * dz).sum(), [w, gamma, beta])
    G, gs = bb.dw_sd_wgrad_loops(dz.numpy(), x.numpy(), 2, 1)
    got_dw, _, got_dgamma, got_dbeta = bc.bn_chain(G, gs, w.detach().numpy(), np.zeros(Cn), gamma.detach().numpy(), mean.numpy(), var.numpy())
    for got, want in ((got_dw, dw), (got_dgamma, dgamma), (got_dbeta, dbeta)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))


def test_scope_all_layout_and_parameter_groups():
    assert _lib.TRAIN_ALL == 2 and _lib.train_scope("all") == 2 and _lib.train_scope_name("all") == "all"
    assert _lib.train_scope(_lib.TRAIN_CPM) == 1 and _lib.train_scope_name(0) == "stages"      # the first two scopes keep their numbers
    for nref, Cn, NH, NP in ((1, 128, 19, 38), (2, 32, 6, 8), (0, 32, 19, 38)):
        sd = synth.make_state_dict(nref, seed=1, num_channels=Cn, num_heatmaps=NH, num_pafs=NP)
        cpm_spec, cpm_total = _lib.train_grad_spec("cpm", nref, Cn, NH, NP)
        spec, total = _lib.train_grad_spec("all", nref, Cn, NH, NP)
        want = ["model.0.0.weight", "model.0.1.weight", "model.0.1.bias"]
        for i in range(1, 12):
            want += ["model.%d.0.weight" % i, "model.%d.1.weight" % i, "model.%d.1.bias" % i,
                     "model.%d.3.weight" % i, "model.%d.4.weight" % i, "model.%d.4.bias" % i]
        assert len(want) == 69 and bb.backbone_keys(sd) == want
        assert [k for k, _, _ in spec] == want + cc.grad_keys(sd) == bb.grad_keys(sd)
        assert [k for k in sd if "running_" not in k and "num_batches_tracked" not in k] == [k for k, _, _ in spec]      # state-dict order, every parameter
        off = 0
        for k, shape, o in spec:
            assert tuple(sd[k].shape) == shape and o == off, k
            off += int(np.prod(shape))
        assert off == total
        by = dict((k, s) for k, s, _ in spec)
        assert by["model.0.0.weight"] == (32, 3, 3, 3) and by["model.2.0.weight"] == (64, 1, 3, 3) and by["model.11.3.weight"] == (512, 512, 1, 1)
        bb_total = sum(int(np.prod(s)) for k, s, _ in spec if k.startswith("model."))
        assert total == bb_total + cpm_total
        assert [(k, s, o - bb_total) for k, s, o in spec[69:]] == cpm_spec                      # the unchanged tail, shifted
        groups = _lib.train_adam_groups("all", nref, Cn, NH, NP)
        assert [k for k, _, _ in groups] == [k for k, _, _ in spec]
        assert groups[69:] == _lib.train_adam_groups("cpm", nref, Cn, NH, NP)
        g = dict((k, (m, wd)) for k, m, wd in groups)
        assert g["model.0.0.weight"] == (1, True) and g["model.0.1.weight"] == (1, False) and g["model.0.1.bias"] == (2, False)
        for i in range(1, 12):
            assert g["model.%d.0.weight" % i] == (1, False) and g["model.%d.3.weight" % i] == (1, True), i
            assert g["model.%d.1.weight" % i] == g["model.%d.4.weight" % i] == (1, False), i
            assert g["model.%d.1.bias" % i] == g["model.%d.4.bias" % i] == (2, False), i
        assert all(bb.group_of(k) == (m, wd) for k, m, wd in groups)
    for bare in (2, 3):                          # Python names the later scopes: a bare number that was an error stays one
        with pytest.raises(ValueError):
            _lib.train_grad_spec(bare, 1, 128, 19, 38)


def test_argument_checks_without_a_handle():
    L = _lib.lib()
    total = C.c_int64()
    assert L.lwp_train_grad_count(_lib.TRAIN_ALL, 1, 128, 19, 38, C.byref(total)) == 69 + 10 + len(_lib.stage_grad_spec(1, 128, 19, 38)[0])
    assert L.lwp_train_grad_count(3, 1, 128, 19, 38, C.byref(total)) == _lib.LWP_ERR_ARG
    assert L.lwp_train_grad_count(_lib.TRAIN_ALL, -1, 128, 19, 38, C.byref(total)) == _lib.LWP_ERR_ARG
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd, off, mult, wd = C.c_int(), C.c_int64(), C.c_int(), C.c_int()
    assert L.lwp_train_grad_spec(_lib.TRAIN_ALL, 1, 128, 19, 38, 0, name, 256, shape, C.byref(nd), C.byref(off)) == _lib.LWP_OK
    assert name.value == b"model.0.0.weight" and off.value == 0 and nd.value == 4
    assert L.lwp_train_grad_spec(_lib.TRAIN_ALL, 1, 128, 19, 38, 10 ** 6, name, 256, shape, C.byref(nd), C.byref(off)) == _lib.LWP_ERR_ARG
    assert L.lwp_train_grad_spec(_lib.TRAIN_ALL, 1, 128, 19, 38, 0, name, 4, shape, C.byref(nd), C.byref(off)) == _lib.LWP_ERR_ARG
    assert L.lwp_train_grad_spec(_lib.TRAIN_ALL, 1, 128, 19, 38, 0, None, 256, shape, C.byref(nd), C.byref(off)) == _lib.LWP_ERR_ARG
    assert L.lwp_train_adam_group(_lib.TRAIN_ALL, 1, 128, 19, 38, 0, C.byref(mult), C.byref(wd)) == _lib.LWP_OK and (mult.value, wd.value) == (1, 1)
    assert L.lwp_train_adam_group(_lib.TRAIN_ALL, 1, 128, 19, 38, -1, C.byref(mult), C.byref(wd)) == _lib.LWP_ERR_ARG
    assert L.lwp_train_adam_group(_lib.TRAIN_ALL, 1, 128, 19, 38, 0, None, C.byref(wd)) == _lib.LWP_ERR_ARG
    assert L.lwp_set_train_scope(None, _lib.TRAIN_ALL) == _lib.LWP_ERR_ARG                       # h == NULL
    assert L.lwp_train_backward(None, None, None, None, 1, 1, 1, 1, C.c_double(1.0), 0, None, None, None) == _lib.LWP_ERR_ARG
