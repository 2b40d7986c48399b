"""Backbone backward on the GPU (-m gpu): train scope "all" of lwp_train_forward / lwp_train_backward / lwp_stage_adam_step against the
float64 restatement of tests/backbone_backward_cases.py, which differentiates the branch the device took (ReLU masks from the
retained activations, within backward_cases' cap) from the image on.

The bar of a gradient tensor g is that of tests/test_gpu_backward.py: e(g) = max|g - g64| / max|g64| <= 8 e_ref, e_ref the
largest e of torch's fp32 CPU autograd over the same restatement on the same inputs against float64 on the fp32 run's own masks.
Kernels alone: a float32 sum of `depth` exact products is within (depth + 8) 2^-24 sum|terms| of the float64 loop statement.
Adam: 1 float32 ulp of the float64 restatement (tests/optim_cases.py).  Repack: the blob lwp_load_weights packs, byte for byte."""
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, optim, synth, val
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import backbone_backward_cases as bb
import backward_cases as bc
import cpm_backward_cases as cc
import optim_cases as oc
import train_cases as tc

pytestmark = pytest.mark.gpu
NET_TOL = 1e-3            # the per-layer parity bound of tests/test_gpu_parity.py
BASE_LR = 4e-5
U = 2.0 ** -24
_runs = {}


def inputs(name, cases=bb.CASES):
    c = cases[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, NH, NP, sd, x


def make_engine(name, scope="all", sd=None, dtype=_lib.F32):
    c, NH, NP, sd0, x = inputs(name)
    eng = Engine(0, nref=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP, dtype=dtype)
    if scope is not None:
        eng.set_train_scope(scope)
    eng.load_state_dict(sd0 if sd is None else sd)
    return eng, c, sd0, x


def targets(eng, c):
    """Targets and loss mask on the network's own map size (8 hs x 8 ws covers the frame where it is no multiple of 8)."""
    hs, ws = bb.map_dims(c)
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (8 * hs, 8 * ws))
    return km, pm, torch.from_numpy(bb.loss_mask(c)).cuda()


def blob_of(eng):
    t = torch.empty(eng.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    eng.export_weights(t)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def merged(sd, params):
    out = dict(sd)
    out.update({k: v.detach().cpu().reshape(sd[k].shape) for k, v in params.items()})
    return out


def stage_acts(eng):
    layers = eng.layers()
    first = [i["index"] for i in layers if i["name"] == "cpm.conv"][0]
    return {i["index"]: eng.train_activation(i["index"]) for i in layers if i["index"] >= first}


class fuse_env(object):
    """LWP_FUSE_DWPW for the engines created inside ("0": depthwise + 1x1 as two layers); None leaves the environment alone."""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get("LWP_FUSE_DWPW")
        if self.value is not None:
            os.environ["LWP_FUSE_DWPW"] = self.value

    def __exit__(self, *exc):
        if self.value is not None:
            if self.saved is None:
                del os.environ["LWP_FUSE_DWPW"]
            else:
                os.environ["LWP_FUSE_DWPW"] = self.saved


def run(name, fuse_dwpw=None):
    """Engine in scope "all", device results and both references of a case, computed once."""
    if (name, fuse_dwpw) in _runs:
        return _runs[(name, fuse_dwpw)]
    with fuse_env(fuse_dwpw):
        eng, c, sd, x = make_engine(name)
    xc = torch.from_numpy(x).cuda()
    km, pm, mask = targets(eng, c)
    fwd = eng.forward(xc)
    outs = eng.train_forward(xc)
    grads, dfeat, dback = eng.stage_backward(km, pm, mask, want_backbone=True)
    torch.cuda.synchronize()
    layers = eng.layers()
    acts = stage_acts(eng)
    cacts = eng.cpm_activations()
    bacts = eng.backbone_activations()
    masks = cc.stage_masks(layers, acts)
    masks["cpm.align"] = torch.from_numpy(cacts["cpm.align"]) > 0
    masks["cpm.conv"] = torch.from_numpy(cacts["cpm"]) > 0
    for nm in bb.RELU_LAYERS:
        masks[nm] = torch.from_numpy(bacts[nm]) > 0
    args = (sd, torch.from_numpy(x), c["nref"], km.cpu(), pm.cpu(), mask.cpu(), c["N"])
    g64, taps64, outs64, acts64 = bb.gradients(*args, masks=masks)
    g32, taps32, _, _ = bb.gradients(*args, dtype=torch.float32)
    g64_32, _, _, _ = bb.gradients(*args, masks=bc.own_masks(taps32))
    e_ref = max(bc.err(g32[k], g64_32[k]) for k in g64_32)
    r = dict(c=c, sd=sd, x=x, xc=xc, eng=eng, km=km, pm=pm, mask=mask, fwd=fwd, outs=outs, grads=grads, dfeat=dfeat, dback=dback,
             acts=acts, cacts=cacts, bacts=bacts, masks=masks, g64=g64, taps64=taps64, acts64=acts64, e_ref=e_ref, layers=layers)
    _runs[(name, fuse_dwpw)] = r
    return r


CASE_NAMES = ["s", "t", "u", "v", "w"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_outputs_are_those_of_forward_and_retained_activations_match_the_restatement(name):
    r = run(name)
    assert len(r["outs"]) == 2 * (r["c"]["nref"] + 1)
    for a, b in zip(r["outs"], r["fwd"]):
        assert tuple(a.shape[2:]) == bb.map_dims(r["c"])
        assert torch.equal(a, b)
    assert list(r["bacts"]) == bb.RELU_LAYERS
    got = dict(r["bacts"])
    got.update((nm, r["cacts"][nm]) for nm in cc.ACT_NAMES)
    assert np.array_equal(r["cacts"]["model.11"], r["bacts"]["model.11"])
    worst = 0.0
    for nm in bb.RELU_LAYERS + cc.ACT_NAMES:
        ref = r["acts64"][nm].numpy()
        assert got[nm].shape == ref.shape, nm
        d = np.abs(got[nm] - ref).max()
        worst = max(worst, d / max(1.0, np.abs(ref).max()))
        assert d <= NET_TOL * max(1.0, np.abs(ref).max()), nm
    print("case %s: retained activations, worst max|diff| / max(1, max|ref|) %.3g" % (name, worst))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_against_float64(name):
    r = run(name)
    bc.check_mask_deviation(r["masks"], r["taps64"])
    assert set(bb.RELU_LAYERS) | set(cc.RELU_LAYERS) <= set(r["taps64"])
    assert list(r["grads"]) == bb.grad_keys(r["sd"])
    got = dict(r["grads"], d_features=r["dfeat"], d_backbone=r["dback"])
    worst, worst_key = 0.0, None
    for k in got:
        assert tuple(got[k].shape) == tuple(r["g64"][k].shape), k
        e = bc.err(got[k].cpu(), r["g64"][k])
        if e > worst:
            worst, worst_key = e, k
    print("case %s: worst e %.3g (%s), e_ref %.3g, ratio %.3g, bar %.3g" % (name, worst, worst_key, r["e_ref"], worst / r["e_ref"], 8 * r["e_ref"]))
    for k in got:
        assert bc.err(got[k].cpu(), r["g64"][k]) <= 8 * r["e_ref"], k
    if name == "w":          # several pixel ranges per weight gradient
        by = dict((i["name"], i["index"]) for i in r["layers"])
        assert r["eng"].backward_splits(by["model.0"]) > 1
        dws = [i["index"] for i in r["layers"] if i["name"].startswith("model.") and i["name"] != "model.0"
               and (i["name"].endswith(".dw") or ("model.%s.dw" % i["name"].split(".")[1]) not in by)]
        assert len(dws) == 11 and min(r["eng"].backward_splits(i, depthwise=True) for i in dws) > 1


@pytest.mark.parametrize("name", ["t", "v"])
def test_gradients_with_unfused_backbone_blocks(name):
    """LWP_FUSE_DWPW=0: every backbone block is a depthwise layer and a 1x1 layer (the default graph fuses all eleven), so the
    depthwise output is retained directly and the 1x1 data gradient reads the blob's folded matrix.  Same bar."""
    r = run(name, "0")
    names = [i["name"] for i in r["layers"] if i["name"].startswith("model.")]
    assert len(names) == 23 and "model.7.dw" in names, names
    assert len([i for i in run(name)["layers"] if i["name"].startswith("model.")]) == 12
    for a, b in zip(r["outs"], r["fwd"]):
        assert torch.equal(a, b)
    for nm in bb.RELU_LAYERS:
        ref = r["acts64"][nm].numpy()
        assert np.abs(r["bacts"][nm] - ref).max() <= NET_TOL * max(1.0, np.abs(ref).max()), nm
    bc.check_mask_deviation(r["masks"], r["taps64"])
    got = dict(r["grads"], d_features=r["dfeat"], d_backbone=r["dback"])
    assert list(r["grads"]) == bb.grad_keys(r["sd"])
    errs = dict((k, bc.err(got[k].cpu(), r["g64"][k])) for k in got)
    worst = max(errs, key=errs.get)
    print("case %s, unfused: worst e %.3g (%s), e_ref %.3g, ratio %.3g" % (name, errs[worst], worst, r["e_ref"], errs[worst] / r["e_ref"]))
    for k in got:
        assert errs[k] <= 8 * r["e_ref"], k


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cpm_and_stage_results_are_those_of_scope_cpm(name):
    """The backbone chain only consumes the gradient at the cpm's input: everything behind it has the bits of scope "cpm"."""
    r = run(name)
    eng1, c, sd, x = make_engine(name, scope="cpm")
    outs1 = eng1.train_forward(r["xc"])
    g1, d1, b1 = eng1.stage_backward(r["km"], r["pm"], r["mask"], want_backbone=True)
    assert list(g1) == cc.grad_keys(sd) and g1
    for k in g1:
        assert torch.equal(g1[k], r["grads"][k]), k
    assert torch.equal(d1, r["dfeat"]) and torch.equal(b1, r["dback"])
    for a, b in zip(outs1, r["outs"]):
        assert torch.equal(a, b)
    acts1, cacts1 = stage_acts(eng1), eng1.cpm_activations()
    assert set(acts1) == set(r["acts"]) and set(cacts1) == set(r["cacts"])
    for k in acts1:
        assert np.array_equal(acts1[k], r["acts"][k]), k
    for k in cacts1:
        assert np.array_equal(cacts1[k], r["cacts"][k]), k


@pytest.mark.parametrize("name", ["s", "v"])
def test_repeatability_and_accumulation(name):
    r = run(name)
    eng = r["eng"]
    flat = eng.flat_of(r["grads"]).clone()
    eng.train_forward(r["xc"])
    g, d, b = eng.stage_backward(r["km"], r["pm"], r["mask"], want_backbone=True)
    assert torch.equal(eng.flat_of(g), flat) and torch.equal(d, r["dfeat"]) and torch.equal(b, r["dback"])      # same inputs, same bits
    g, d = eng.stage_backward(r["km"], r["pm"], r["mask"], loss_scale=0.5)
    acc = eng.flat_of(g)
    assert torch.equal(acc, flat * 0.5) and torch.equal(d, r["dfeat"] * 0.5)
    eng.stage_backward(r["km"], r["pm"], r["mask"], loss_scale=0.5, into=acc)
    assert torch.equal(acc, flat)                                          # two halves accumulated: one full run, exactly


# ---------------------------------------------------------------------------------------------- the new kernels alone
@pytest.mark.parametrize("s,d", [(1, 1), (2, 1), (1, 2), (2, 2)])
def test_depthwise_gradient_kernels_against_the_loop_statements(s, d):
    """Crafted tensors: odd and even maps, a map smaller than the dilated kernel, 68 channels (a second, ragged channel group),
    pixel ranges of 16 so that every shape takes several."""
    eng, _, _, _ = make_engine("u", scope=None)
    g = torch.Generator().manual_seed(51 + 2 * s + d)
    for N, Cn, H, W in ((2, 8, 5, 7), (1, 68, 9, 6), (1, 4, 2, 3), (3, 4, 8, 8)):
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        x = torch.randn(N, Cn, H, W, generator=g)
        w = torch.randn(Cn, 1, 3, 3, generator=g)
        dz = torch.randn(N, Cn, Ho, Wo, generator=g)
        dx, G, gs, splits = eng.debug_dw_grad(dz.cuda(), x.cuda(), w.cuda(), s, d, max_chunk=16)
        assert splits == (N * Ho * Wo + 15) // 16
        x64, w64, dz64 = x.double().numpy(), w.double().numpy(), dz.double().numpy()
        want_dx = bb.dw_sd_dgrad_loops(dz64, w64, H, W, s, d)
        want_G, want_g = bb.dw_sd_wgrad_loops(dz64, x64, s, d)
        abs_dx = bb.dw_sd_dgrad_loops(np.abs(dz64), np.abs(w64), H, W, s, d)
        abs_G, abs_g = bb.dw_sd_wgrad_loops(np.abs(dz64), np.abs(x64), s, d)
        depth = N * Ho * Wo
        assert (np.abs(dx.cpu().double().numpy() - want_dx) <= (9 + 8) * U * abs_dx).all(), (N, Cn, H, W)
        assert (np.abs(G.cpu().double().numpy() - want_G) <= (depth + 8) * U * abs_G).all(), (N, Cn, H, W)
        assert (np.abs(gs.cpu().double().numpy() - want_g) <= (depth + 8) * U * abs_g).all(), (N, Cn, H, W)
        dx2, G2, gs2, _ = eng.debug_dw_grad(dz.cuda(), x.cuda(), w.cuda(), s, d, max_chunk=16)
        assert torch.equal(dx, dx2) and torch.equal(G, G2) and torch.equal(gs, gs2)


def test_stem_weight_gradient_kernel_against_the_loop_statement():
    eng, _, _, _ = make_engine("u", scope=None)
    g = torch.Generator().manual_seed(61)
    for N, H, W, chunk in ((2, 9, 7, 5), (1, 8, 8, 0), (1, 30, 20, 64)):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        x = torch.randn(N, 3, H, W, generator=g)
        dz = torch.randn(N, 32, Ho, Wo, generator=g)
        G, gs, splits = eng.debug_stem_wgrad(dz.cuda(), x.cuda(), max_chunk=chunk)
        depth = N * Ho * Wo
        assert splits == ((depth + chunk - 1) // chunk if chunk else 1)
        want_G, want_g = bb.stem_wgrad_loops(dz.double().numpy(), x.double().numpy())
        abs_G, abs_g = bb.stem_wgrad_loops(np.abs(dz.double().numpy()), np.abs(x.double().numpy()))
        assert (np.abs(G.cpu().double().numpy() - want_G) <= (depth + 8) * U * abs_G).all(), (N, H, W)
        assert (np.abs(gs.cpu().double().numpy() - want_g) <= (depth + 8) * U * abs_g).all(), (N, H, W)
        G2, gs2, _ = eng.debug_stem_wgrad(dz.cuda(), x.cuda(), max_chunk=chunk)
        assert torch.equal(G, G2) and torch.equal(gs, gs2)


# ---------------------------------------------------------------------------------------------- Adam and repack
def test_adam_on_all_scope_entries_within_one_ulp_of_float64():
    eng, c, sd, _ = make_engine("s")
    spec, total = eng.grad_spec()
    assert [k for k, _, _ in spec] == bb.grad_keys(sd)
    assert eng.adam_groups() == [(k,) + bb.group_of(k) for k, _, _ in spec]
    lr, decay = bb.flat_groups(spec, BASE_LR)
    n_bb = sum(int(np.prod(s)) for k, s, _ in spec if k.startswith("model."))
    worst, differing = 0, 0
    for t in range(1, 4):
        p0 = eng.flat_of(eng.stage_params()).cpu().numpy()
        st = eng.adam_state()
        assert st["step"] == t - 1
        m0, v0 = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
        g = oc.crafted_gradients(spec, t)
        eng.adam_step(torch.from_numpy(g).cuda(), BASE_LR, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
        st = eng.adam_state()
        got = (eng.flat_of(eng.stage_params()).cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        want = oc.adam_ref(p0, g, m0, v0, t, lr, decay)
        for a, w in zip(got, want):
            assert np.isfinite(a).all()
            dist = oc.ulp_distance(a, w.astype(np.float32))
            worst = max(worst, int(dist.max()))
            differing += int((dist[:n_bb] != 0).sum())
        if t == 1:
            for k, shape, off in spec:
                assert np.array_equal(p0[off:off + int(np.prod(shape))].reshape(shape), sd[k].numpy()), k     # the raw values as loaded
    print("all scope, case s: %d elements (%d of the backbone) x 3 arrays x 3 steps, worst %d ulp, %d backbone values not identical"
          % (total, n_bb, worst, differing))
    assert worst <= 1


_steps = {}


def stepped(name, fuse_dwpw=None):
    """Case engine (scope "all") after one step IMMEDIATELY followed by a forward, and the fresh engine given the same values
    through lwp_load_weights.  fuse_dwpw "0": both engines are created under LWP_FUSE_DWPW=0 (depthwise + 1x1 as two layers)."""
    key = (name, fuse_dwpw)
    if key in _steps:
        return _steps[key]
    with fuse_env(fuse_dwpw):
        eng, c, sd, x = make_engine(name)
        kinds = [i["name"] for i in eng.layers() if i["name"].startswith("model.")]
        xc = torch.from_numpy(x).cuda()
        before = blob_of(eng)
        eng.forward(xc)
        total = eng.grad_spec()[1]
        g = torch.from_numpy(np.random.RandomState(c["seed"]).standard_normal(total).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        eng.adam_step(g, 1e-2, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
        outs = eng.forward(xc)
        params = eng.trained_params()
        fresh, _, _, _ = make_engine(name, sd=merged(sd, params))
    r = dict(eng=eng, fresh=fresh, sd=sd, xc=xc, before=before, outs=outs, params=params, c=c, kinds=kinds)
    _steps[key] = r
    return r


@pytest.mark.parametrize("name,fuse", [("s", None), ("v", None), ("s", "0")])
def test_repacked_blob_is_the_blob_load_weights_packs(name, fuse):
    """The default graph runs every backbone block as one fused launch (12 backbone layers with the stem); LWP_FUSE_DWPW=0
    splits them all (23)."""
    r = stepped(name, fuse)
    assert len(r["kinds"]) == (23 if fuse == "0" else 12), r["kinds"]
    got, want = blob_of(r["eng"]), blob_of(r["fresh"])
    assert got.shape == want.shape == r["before"].shape
    assert not np.array_equal(got, r["before"])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "first differing byte %d of %d" % (diff[0], got.size)
    assert list(r["params"]) == bb.grad_keys(r["sd"])
    for k, v in r["params"].items():                                       # the step moved every parameter
        assert not torch.equal(v.cpu().reshape(r["sd"][k].shape), r["sd"][k]), k


@pytest.mark.parametrize("name", ["s", "v"])
def test_forward_behind_the_step_is_the_fresh_handles(name):
    r = stepped(name)
    want = r["fresh"].forward(r["xc"])
    assert len(want) == len(r["outs"]) == 2 * (r["c"]["nref"] + 1)
    for a, b in zip(r["outs"], want):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- training and scope rules
def make_net(name="d"):
    c, NH, NP, sd, x = inputs(name, bc.CASES)
    net = PoseEstimationWithMobileNet(num_refinement_stages=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    K = tc.skeleton(c["skel"])[0]
    kp, n = bc.persons(c)
    labels = tc.frames_to_labels([[kp[f, i] for i in range(n[f])] for f in range(c["N"])], K)
    full = np.repeat(np.repeat(bc.loss_mask(c), 8, 1), 8, 2)
    return net, sd, x, labels, full


def test_twenty_steps_in_all_scope_lower_the_loss_of_case_d():
    net, sd, x, labels, full = make_net()
    opt = optim.StageAdam(net, base_lr=oc.LOOP_LR, weight_decay=oc.WEIGHT_DECAY, scope="all")
    assert opt.scope == "all" and net.engine.train_scope == "all"
    losses = [sum(val.train_step(net, opt, x, labels, full)) for _ in range(oc.LOOP_STEPS)]
    losses.append(sum(val.stage_losses(net, x, labels, full)))
    print("all scope, case d: loss %.9g -> %.9g" % (losses[0], losses[-1]))
    assert opt.steps == oc.LOOP_STEPS
    assert losses[-1] < losses[0]
    after = net.state_dict()
    for k in sd:
        if not k.startswith("model."):
            continue
        if "running_" in k or "num_batches_tracked" in k:
            assert torch.equal(after[k].cpu(), sd[k]), k                   # the statistics as loaded, bit for bit
        else:
            assert not torch.equal(after[k].cpu(), sd[k]), k               # every conv weight, BatchNorm weight and bias has moved
    ck = opt.state_dict()
    assert ck["step"] == oc.LOOP_STEPS and list(ck["exp_avg"]) == bb.grad_keys(sd)
    # a checkpoint resumed in a second engine reproduces the next step bit for bit
    net2, _, _, _, _ = make_net()
    net2.load_state_dict(after)
    opt2 = optim.StageAdam(net2, base_lr=oc.LOOP_LR, weight_decay=oc.WEIGHT_DECAY, scope="all")
    opt2.load_state_dict(ck)
    l1 = val.train_step(net, opt, x, labels, full)
    l2 = val.train_step(net2, opt2, x, labels, full)
    assert l1 == l2
    p1, p2 = net.engine.stage_params(), net2.engine.stage_params()
    for k in p1:
        assert torch.equal(p1[k], p2[k]), k
    # narrowing to "cpm" keeps the trained backbone readable
    trained = {k: v.cpu().clone() for k, v in p1.items()}
    net.engine.load_adam_state(None)
    optim.StageAdam(net, base_lr=oc.LOOP_LR, scope="cpm")
    assert net.engine.train_scope == "cpm" and list(net.engine.stage_params()) == cc.grad_keys(sd)
    got = net.state_dict()
    for k in bb.backbone_keys(sd):
        assert torch.equal(got[k].cpu(), trained[k].reshape(sd[k].shape)), k
    with pytest.raises(Exception):
        net.train(True)


def test_scope_rules():
    c, NH, NP, sd, x = inputs("s")
    half = Engine(0, nref=1, num_channels=64, dtype=_lib.F16)
    with pytest.raises(ValueError, match="fp32"):
        half.set_train_scope("all")
    eng, _, _, _ = make_engine("s")
    xc = torch.from_numpy(x).cuda()
    total = eng.grad_spec()[1]
    eng.adam_step(torch.ones(total, device="cuda"), BASE_LR, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
    with pytest.raises(RuntimeError, match="lwp_stage_adam_reset"):
        eng.set_train_scope("cpm")
    assert eng.train_scope == "all"
    # "stages" after "all" on a fresh optimiser: the gradients of an engine that was never widened, bit for bit
    wide, _, _, _ = make_engine("s")
    wide.train_forward(xc)
    km, pm, mask = targets(wide, c)
    wide.stage_backward(km, pm, mask)
    wide.set_train_scope("stages")
    never, _, _, _ = make_engine("s", scope="stages")
    got, want = [], []
    for e, dst in ((wide, got), (never, want)):
        e.train_forward(xc)
        dst.extend(e.stage_backward(km, pm, mask))
    assert list(got[0]) == list(want[0]) == bc.grad_keys(sd)
    for k in want[0]:
        assert torch.equal(got[0][k], want[0][k]), k
    assert torch.equal(got[1], want[1])
