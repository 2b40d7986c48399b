"""CPU: the float64 restatement the stage-backward tests differentiate (tests/backward_cases.py) against the oracle's forward,
its masked ReLU against plain autograd, the BatchNorm chain rule the device mirrors, and the new exports."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from oracle import net_ref

import backward_cases as bc
import train_cases as tc


def case_inputs(name):
    """(sd, x, feat64, outs64, keypoint_maps, paf_maps, mask) of a case on the CPU, targets from the NumPy restatement."""
    c = bc.CASES[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    taps = {}
    outs = net_ref.forward64(sd, torch.from_numpy(x), c["nref"], taps)
    K, lk, lp = tc.skeleton(c["skel"])
    kp, n = bc.persons(c)
    km, pm = tc.targets(kp, n, c["H"], c["W"], 8, 7, 1, K, tc.limb_rows(lk, lp))
    return sd, x, taps["cpm"], outs, torch.from_numpy(km), torch.from_numpy(pm), torch.from_numpy(bc.loss_mask(c))


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_restatement_equals_the_oracle_forward(name):
    c = bc.CASES[name]
    sd, x, feat, outs, km, pm, mask = case_inputs(name)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    got = bc.stages(sd64, feat, c["nref"])
    assert len(got) == len(outs) == 2 * (c["nref"] + 1)
    for g, o in zip(got, outs):
        assert g.shape == o.shape
        assert float((g - o).abs().max()) <= 1e-12 * float(o.max() - o.min())


@pytest.mark.parametrize("name", ["a", "b", "d", "n8"])
def test_own_masks_reproduce_plain_relu_autograd_and_fp32_stays_on_the_branch(name):
    c = bc.CASES[name]
    sd, x, feat, outs, km, pm, mask = case_inputs(name)
    args = (sd, feat, c["nref"], km, pm, mask, c["N"])
    plain, taps, _ = bc.gradients(*args)
    masked, _, _ = bc.gradients(*args, masks=bc.own_masks(taps))
    assert set(plain) == set(masked) and "d_features" in plain
    assert not any("running_" in k or "num_batches" in k for k in plain)
    for k in plain:
        assert torch.equal(plain[k], masked[k]), k
    # the seed keeps torch's fp32 forward (the device's stand-in) within the cap on branch deviations
    _, taps32, _ = bc.gradients(*args, dtype=torch.float32)
    bc.check_mask_deviation(bc.own_masks(taps32), taps)
    g32, _, _ = bc.gradients(*args, dtype=torch.float32)
    g64, _, _ = bc.gradients(*args, masks=bc.own_masks(taps32))
    e_ref = max(bc.err(g32[k], g64[k]) for k in g64)
    print("case %s: e_ref %.3g" % (name, e_ref))
    assert e_ref < 1e-4


def test_bn_chain_rule_equals_autograd():
    """Folded (what the kernels differentiate) against unfolded (what the user holds) conv + BatchNorm, float64."""
    g = torch.Generator().manual_seed(5)
    co, ci = 6, 5
    x = torch.randn(2, ci, 7, 6, dtype=torch.float64, generator=g)
    W = torch.randn(co, ci, 3, 3, dtype=torch.float64, generator=g).requires_grad_(True)
    b = torch.randn(co, dtype=torch.float64, generator=g).requires_grad_(True)
    gamma = (torch.rand(co, dtype=torch.float64, generator=g) + 0.5).requires_grad_(True)
    beta = torch.randn(co, dtype=torch.float64, generator=g).requires_grad_(True)
    mean = torch.randn(co, dtype=torch.float64, generator=g)
    var = torch.rand(co, dtype=torch.float64, generator=g) + 0.5
    up = torch.randn(2, co, 7, 6, dtype=torch.float64, generator=g)
    y = F.relu(F.batch_norm(F.conv2d(x, W, b, 1, 2, 2), mean, var, gamma, beta, False, 0.0, 1e-5))
    want = torch.autograd.grad((y * up).sum(), [W, b, gamma, beta])
    s = (gamma / torch.sqrt(var + 1e-5)).detach()
    Wf = (W.detach() * s.view(-1, 1, 1, 1)).requires_grad_(True)
    bf = ((b.detach() - mean) * s + beta.detach()).requires_grad_(True)
    yf = F.relu(F.conv2d(x, Wf, bf, 1, 2, 2))
    G, gb = torch.autograd.grad((yf * up).sum(), [Wf, bf])
    got = bc.bn_chain(G.numpy(), gb.numpy(), W.detach().numpy(), b.detach().numpy(), gamma.detach().numpy(), mean.numpy(), var.numpy())
    for a, w in zip(got, want):
        assert np.abs(a - w.numpy()).max() <= 1e-12 * max(1.0, float(w.abs().max()))


def test_new_exports_and_gradient_layout():
    for name in ("lwp_train_forward", "lwp_stage_backward", "lwp_stage_grad_count", "lwp_stage_grad_spec",
                 "lwp_debug_train_activation", "lwp_debug_backward_splits", "lwp_profile_stage_backward"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    for nref, C, NH, NP in ((1, 128, 19, 38), (2, 32, 6, 8), (0, 32, 19, 38)):
        spec, total = _lib.stage_grad_spec(nref, C, NH, NP)
        sd = synth.make_state_dict(nref, seed=1, num_channels=C, num_heatmaps=NH, num_pafs=NP)
        assert [k for k, _, _ in spec] == bc.grad_keys(sd)           # state-dict (= lwp_param_spec) order, no running_* keys
        off = 0
        for k, shape, o in spec:
            assert tuple(sd[k].shape) == shape and o == off
            off += int(np.prod(shape))
        assert off == total
