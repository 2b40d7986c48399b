"""CPU: the restatement the cpm-backward tests differentiate (tests/cpm_backward_cases.py) against the oracle's forward taps, the
ELU derivative taken from the output, the tap / offset convention of the depthwise gradient kernels, the branch cap of the two
cpm ReLUs with torch's fp32 forward as the device's stand-in, and the gradient layout and parameter groups of train scope "cpm"."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from oracle import net_ref

import backward_cases as bc
import cpm_backward_cases as cc
import train_cases as tc


def case_inputs(name):
    c = cc.CASES[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, sd, x


@pytest.mark.parametrize("name", ["a", "b", "d", "f", "g"])
def test_restatement_equals_the_oracle_taps(name):
    c, sd, x = case_inputs(name)
    taps = {}
    net_ref.forward64(sd, torch.from_numpy(x), c["nref"], taps, stop_after="cpm")
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    acts = {}
    cc.cpm(sd64, taps["model.11"], acts=acts)
    assert list(acts) == cc.ACT_NAMES
    for nm in cc.ACT_NAMES:
        o = taps[nm]
        assert acts[nm].shape == o.shape, nm
        assert float((acts[nm] - o).abs().max()) <= 1e-12 * float(o.max() - o.min()), nm


def test_elu_derivative_from_the_output():
    g = torch.Generator().manual_seed(7)
    z = (torch.randn(4096, dtype=torch.float64, generator=g) * 3).requires_grad_(True)
    with torch.no_grad():
        z[:8] = torch.tensor([0.0, -0.0, 1e-300, -1e-300, 1e-9, -1e-9, 40.0, -40.0], dtype=torch.float64)
    up = torch.randn(4096, dtype=torch.float64, generator=g)
    y = F.elu(z)
    (want,) = torch.autograd.grad((y * up).sum(), [z])
    yd = y.detach()
    got = up * torch.where(yd > 0, torch.ones_like(yd), yd + 1)
    assert float((got - want).abs().max()) <= 1e-15 * float(want.abs().max())


def test_depthwise_gradient_formulas_equal_autograd():
    """Ragged toy shape: 5 channels, a 4 x 3 and (every tap of every pixel but the centre outside) a 1 x 1 map."""
    g = torch.Generator().manual_seed(9)
    for N, C, H, W in ((2, 5, 4, 3), (1, 5, 1, 1), (1, 3, 2, 5)):
        x = torch.randn(N, C, H, W, dtype=torch.float64, generator=g).requires_grad_(True)
        w = torch.randn(C, 1, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
        dz = torch.randn(N, C, H, W, dtype=torch.float64, generator=g)
        z = F.conv2d(x, w, None, 1, 1, 1, C)
        dx, dw = torch.autograd.grad((z * dz).sum(), [x, w])
        got_dx = cc.dw_dgrad_loops(dz.numpy(), w.detach().numpy())
        got_dw = cc.dw_wgrad_loops(dz.numpy(), x.detach().numpy())
        assert np.abs(got_dx - dx.numpy()).max() <= 1e-13 * max(1.0, float(dx.abs().max()))
        assert np.abs(got_dw - dw.numpy()).max() <= 1e-13 * max(1.0, float(dw.abs().max()))


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f", "g"])
def test_fp32_forward_stays_on_the_float64_branch(name):
    """The device's stand-in: torch's fp32 CPU forward from net_ref.forward's fp32 model.11.  Its ReLU masks, cpm.align and
    cpm.conv included, are within backward_cases' cap of the float64 restatement's own on the same input."""
    c, sd, x = case_inputs(name)
    taps = {}
    net_ref.forward(sd, torch.from_numpy(x), c["nref"], taps, stop_after="model.11")
    xin = taps["model.11"]
    K, lk, lp = tc.skeleton(c["skel"])
    kp, n = bc.persons(c)
    km, pm = tc.targets(kp, n, c["H"], c["W"], 8, 7, 1, K, tc.limb_rows(lk, lp))
    args = (sd, xin, c["nref"], torch.from_numpy(km), torch.from_numpy(pm), torch.from_numpy(bc.loss_mask(c)), c["N"])
    g32, taps32, _, _ = cc.gradients(*args, dtype=torch.float32)
    _, taps64, _, _ = cc.gradients(*args)
    assert set(cc.RELU_LAYERS) <= set(taps64) and set(taps32) == set(taps64)
    masks32 = bc.own_masks(taps32)
    bc.check_mask_deviation(masks32, taps64)
    if name != "c":          # (the float64 backward of the 46 x 46 maps takes seconds: e_ref of the large case is the GPU test's)
        g64, _, _, _ = cc.gradients(*args, masks=masks32)
        assert set(g64) == set(cc.grad_keys(sd)) | {"d_features", "d_backbone"}
        e_ref = max(bc.err(g32[k], g64[k]) for k in g64)
        print("case %s: e_ref %.3g" % (name, e_ref))
        assert e_ref < 1e-4


def test_scope_layout_and_parameter_groups():
    for name in ("lwp_set_train_scope", "lwp_train_grad_count", "lwp_train_grad_spec", "lwp_train_adam_group", "lwp_train_backward",
                 "lwp_debug_train_copy", "lwp_debug_backward_dw_splits"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    for nref, C, NH, NP in ((1, 128, 19, 38), (2, 32, 6, 8), (0, 32, 19, 38)):
        sd = synth.make_state_dict(nref, seed=1, num_channels=C, num_heatmaps=NH, num_pafs=NP)
        old, old_total = _lib.stage_grad_spec(nref, C, NH, NP)
        assert _lib.train_grad_spec("stages", nref, C, NH, NP) == (old, old_total)              # scope 0: entry for entry
        assert _lib.train_adam_groups("stages", nref, C, NH, NP) == _lib.stage_adam_groups(nref, C, NH, NP)
        spec, total = _lib.train_grad_spec("cpm", nref, C, NH, NP)
        cpm_keys = ["cpm.align.0.weight", "cpm.align.0.bias"] + [k for j in range(3) for k in ("cpm.trunk.%d.0.weight" % j, "cpm.trunk.%d.2.weight" % j)] \
            + ["cpm.conv.0.weight", "cpm.conv.0.bias"]
        assert cc.cpm_keys(sd) == cpm_keys
        assert [k for k, _, _ in spec] == cpm_keys + bc.grad_keys(sd) == cc.grad_keys(sd)
        off = 0
        for k, shape, o in spec:
            assert tuple(sd[k].shape) == shape and o == off, k
            off += int(np.prod(shape))
        assert off == total
        for j in range(3):
            assert dict((k, s) for k, s, _ in spec)["cpm.trunk.%d.0.weight" % j] == (C, 1, 3, 3)
        cpm_total = sum(int(np.prod(s)) for k, s, _ in spec if k.startswith("cpm."))
        assert total == cpm_total + old_total
        assert [(k, s, o - cpm_total) for k, s, o in spec[10:]] == old                          # the unchanged tail, shifted
        groups = _lib.train_adam_groups("cpm", nref, C, NH, NP)
        assert [k for k, _, _ in groups] == [k for k, _, _ in spec]
        assert groups[10:] == _lib.stage_adam_groups(nref, C, NH, NP)
        want = {"cpm.align.0.weight": (1, True), "cpm.align.0.bias": (2, False), "cpm.conv.0.weight": (1, True), "cpm.conv.0.bias": (2, False)}
        for j in range(3):
            want["cpm.trunk.%d.0.weight" % j] = (1, False)
            want["cpm.trunk.%d.2.weight" % j] = (1, True)
        assert dict((k, (m, wd)) for k, m, wd in groups[:10]) == want
        assert all(cc.group_of(k) == (m, wd) for k, m, wd in groups)
    with pytest.raises(ValueError):
        _lib.train_grad_spec(2, 1, 128, 19, 38)
    with pytest.raises(ValueError):
        _lib.train_grad_spec("backbone", 1, 128, 19, 38)
