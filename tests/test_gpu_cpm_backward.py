"""Cpm backward on the GPU (-m gpu): train scope "cpm" of lwp_train_forward / lwp_train_backward / lwp_stage_adam_step against the
float64 restatement of tests/cpm_backward_cases.py, which differentiates the branch the device took (ReLU masks from the
retained activations, within backward_cases' cap) starting from the device's own retained cpm input.

The bar of a gradient tensor g is that of tests/test_gpu_backward.py: e(g) = max|g - g64| / max|g64| <= 8 e_ref, e_ref the
largest e of torch's fp32 CPU autograd over the same restatement on the same inputs against float64 on the fp32 run's own masks.
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

import backward_cases as bc
import cpm_backward_cases as cc
import optim_cases as oc
import train_cases as tc

pytestmark = pytest.mark.gpu
NET_TOL = 1e-3            # the per-layer parity bound of tests/test_gpu_parity.py
BASE_LR = 4e-5
_runs = {}


def inputs(name):
    c = cc.CASES[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, NH, NP, sd, x


def make_engine(name, scope="cpm", sd=None):
    c, NH, NP, sd0, x = inputs(name)
    eng = Engine(0, nref=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    K, lk, lp = tc.skeleton(c["skel"])
    if c["skel"] != "coco":
        eng.set_skeleton(lk, lp, K)
    eng.set_train_scope(scope)
    eng.load_state_dict(sd0 if sd is None else sd)
    return eng, c, sd0, x


def blob_of(eng):
    t = torch.empty(eng.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    eng.export_weights(t)
    torch.cuda.synchronize()
    return t.cpu().numpy()


def merged(sd, params):
    out = dict(sd)
    out.update({k: v.detach().cpu().reshape(sd[k].shape) for k, v in params.items()})
    return out


def run(name):
    """Engine in scope "cpm", device results and both references of a case, computed once."""
    if name in _runs:
        return _runs[name]
    eng, c, sd, x = make_engine(name)
    xc = torch.from_numpy(x).cuda()
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (c["H"], c["W"]))
    mask = torch.from_numpy(bc.loss_mask(c)).cuda()
    fwd = eng.forward(xc)
    outs = eng.train_forward(xc)
    grads, dfeat, dback = eng.stage_backward(km, pm, mask, want_backbone=True)
    torch.cuda.synchronize()
    layers = eng.layers()
    first = [i["index"] for i in layers if i["name"] == "cpm.conv"][0]
    acts = {i["index"]: eng.train_activation(i["index"]) for i in layers if i["index"] >= first}
    cacts = eng.cpm_activations()
    dw_splits = {}
    for i in layers:
        if i["name"].startswith("cpm.trunk."):
            fused = not any(j["name"] == i["name"][:-2] + "dw" for j in layers)
            if i["name"].endswith(".dw") or fused:
                dw_splits[i["name"]] = eng.backward_splits(i["index"], depthwise=True)
    masks = cc.stage_masks(layers, acts)
    masks["cpm.align"] = torch.from_numpy(cacts["cpm.align"]) > 0
    masks["cpm.conv"] = torch.from_numpy(cacts["cpm"]) > 0
    args = (sd, torch.from_numpy(cacts["model.11"]), c["nref"], km.cpu(), pm.cpu(), mask.cpu(), c["N"])
    g64, taps64, outs64, acts64 = cc.gradients(*args, masks=masks)
    g32, taps32, _, _ = cc.gradients(*args, dtype=torch.float32)
    g64_32, _, _, _ = cc.gradients(*args, masks=bc.own_masks(taps32))
    e_ref = max(bc.err(g32[k], g64_32[k]) for k in g64_32)
    r = dict(c=c, sd=sd, x=x, xc=xc, eng=eng, km=km, pm=pm, mask=mask, fwd=fwd, outs=outs, grads=grads, dfeat=dfeat, dback=dback,
             cacts=cacts, dw_splits=dw_splits, masks=masks, g64=g64, taps64=taps64, acts64=acts64, e_ref=e_ref)
    _runs[name] = r
    return r


CASE_NAMES = ["a", "b", "c", "d", "f", "g"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_outputs_are_those_of_forward_and_cpm_activations_match_the_restatement(name):
    r = run(name)
    assert len(r["outs"]) == 2 * (r["c"]["nref"] + 1)
    for a, b in zip(r["outs"], r["fwd"]):
        assert torch.equal(a, b)
    assert set(r["cacts"]) == set(cc.ACT_NAMES) | {"model.11"}
    for nm in cc.ACT_NAMES:
        ref = r["acts64"][nm].numpy()
        got = r["cacts"][nm]
        assert got.shape == ref.shape, nm
        d = np.abs(got - ref).max()
        print("case %s %-18s max|diff| %.3g of %.3g" % (name, nm, d, np.abs(ref).max()))
        assert d <= NET_TOL * max(1.0, np.abs(ref).max()), nm


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_against_float64(name):
    r = run(name)
    bc.check_mask_deviation(r["masks"], r["taps64"])
    assert set(cc.RELU_LAYERS) <= set(r["taps64"])
    assert list(r["grads"]) == cc.grad_keys(r["sd"])
    got = dict(r["grads"], d_features=r["dfeat"], d_backbone=r["dback"])
    worst = 0.0
    for k in sorted(got):
        assert tuple(got[k].shape) == tuple(r["g64"][k].shape), k
        e = bc.err(got[k].cpu(), r["g64"][k])
        worst = max(worst, e)
        print("case %s %-55s e %.3g" % (name, k, e))
    print("case %s: worst e %.3g, e_ref %.3g, ratio %.3g, bar %.3g" % (name, worst, r["e_ref"], worst / r["e_ref"], 8 * r["e_ref"]))
    for k in got:
        assert bc.err(got[k].cpu(), r["g64"][k]) <= 8 * r["e_ref"], k
    assert len(r["dw_splits"]) == 3
    if name == "c":
        assert min(r["dw_splits"].values()) > 1, r["dw_splits"]          # more than one pixel range per depthwise weight gradient


@pytest.mark.parametrize("name", ["a", "b", "f", "g"])
def test_stage_gradients_are_those_of_scope_stages(name):
    """The cpm chain only consumes d_features: the stage gradients and d_features of scope "cpm" have the bits of scope "stages"."""
    r = run(name)
    eng0, c, sd, x = make_engine(name, scope="stages")
    eng0.train_forward(r["xc"])
    g0, d0 = eng0.stage_backward(r["km"], r["pm"], r["mask"])
    assert list(g0) == bc.grad_keys(sd) and g0
    for k in g0:
        assert torch.equal(g0[k], r["grads"][k]), k
    assert torch.equal(d0, r["dfeat"])
    with pytest.raises(ValueError, match="LWP_TRAIN_CPM"):
        eng0.stage_backward(r["km"], r["pm"], r["mask"], want_backbone=True)


@pytest.mark.parametrize("name", ["a", "f"])
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


def test_adam_on_cpm_scope_entries_within_one_ulp_of_float64():
    eng, c, sd, _ = make_engine("a")
    spec, total = eng.grad_spec()
    assert [k for k, _, _ in spec] == cc.grad_keys(sd)
    assert eng.adam_groups() == [(k,) + cc.group_of(k) for k, _, _ in spec]
    lr, decay = cc.flat_groups(spec, BASE_LR)
    worst = 0
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
            worst = max(worst, int(oc.ulp_distance(a, w.astype(np.float32)).max()))
        if t == 1:
            for k, shape, off in spec:
                assert np.array_equal(p0[off:off + int(np.prod(shape))].reshape(shape), sd[k].numpy()), k     # the raw values as loaded
    print("cpm scope, case a: %d elements x 3 arrays x 3 steps, worst %d ulp" % (total, worst))
    assert worst <= 1


_steps = {}


def stepped(name, fuse_dwpw=None):
    """Case engine (scope "cpm") after one step IMMEDIATELY followed by a forward, and the fresh engine given the same values
    through lwp_load_weights.  fuse_dwpw "0": both engines are created under LWP_FUSE_DWPW=0 (depthwise + 1x1 as two layers)."""
    key = (name, fuse_dwpw)
    if key in _steps:
        return _steps[key]
    saved = os.environ.get("LWP_FUSE_DWPW")
    if fuse_dwpw is not None:
        os.environ["LWP_FUSE_DWPW"] = fuse_dwpw
    try:
        eng, c, sd, x = make_engine(name)
        kinds = [i["name"] for i in eng.layers() if i["name"].startswith("cpm.trunk.")]
        xc = torch.from_numpy(x).cuda()
        before = blob_of(eng)
        eng.forward(xc)
        total = eng.grad_spec()[1]
        g = torch.from_numpy(np.random.RandomState(c["seed"]).standard_normal(total).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        eng.adam_step(g, 1e-2, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
        outs = eng.forward(xc)
        params = eng.stage_params()
        fresh, _, _, _ = make_engine(name, sd=merged(sd, params))
    finally:
        if fuse_dwpw is not None:
            if saved is None:
                del os.environ["LWP_FUSE_DWPW"]
            else:
                os.environ["LWP_FUSE_DWPW"] = saved
    r = dict(eng=eng, fresh=fresh, sd=sd, xc=xc, before=before, outs=outs, params=params, c=c, kinds=kinds)
    _steps[key] = r
    return r


@pytest.mark.parametrize("name,fuse", [("a", None), ("g", None), ("a", "0"), ("g", "0")])
def test_repacked_blob_is_the_blob_load_weights_packs(name, fuse):
    """The default graph runs the trunk of case g (128 channels) as three fused blocks and that of case a (32 channels, no fused
    kernel) as depthwise + 1x1 layers; LWP_FUSE_DWPW=0 splits g's blocks too."""
    r = stepped(name, fuse)
    assert len(r["kinds"]) == (3 if (name, fuse) == ("g", None) else 6), r["kinds"]
    got, want = blob_of(r["eng"]), blob_of(r["fresh"])
    assert got.shape == want.shape == r["before"].shape
    assert not np.array_equal(got, r["before"])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "first differing byte %d of %d" % (diff[0], got.size)
    assert list(r["params"]) == cc.grad_keys(r["sd"])
    for k, v in r["params"].items():                                       # the step moved every cpm and stage parameter
        assert not torch.equal(v.cpu().reshape(r["sd"][k].shape), r["sd"][k]), k


def test_forward_behind_the_step_and_scope_state():
    r = stepped("a")
    want = r["fresh"].forward(r["xc"])
    assert len(want) == len(r["outs"]) == 2 * (r["c"]["nref"] + 1)
    for a, b in zip(r["outs"], want):
        assert torch.equal(a, b)
    eng = r["eng"]
    with pytest.raises(RuntimeError, match="lwp_stage_adam_reset"):
        eng.set_train_scope("stages")
    assert eng.train_scope == "cpm" and [k for k, _, _ in eng.grad_spec()[0]] == cc.grad_keys(r["sd"])
    eng.load_adam_state(None)                                              # lwp_stage_adam_reset
    eng.set_train_scope("stages")
    assert eng.train_scope == "stages" and [k for k, _, _ in eng.grad_spec()[0]] == bc.grad_keys(r["sd"])
    for a, b in zip(eng.forward(r["xc"]), want):                           # the weights did not move with the scope
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="scope"):
        eng.set_train_scope("backbone")
    eng.set_train_scope("cpm")
    with pytest.raises(ValueError, match="retaining forward"):            # the scope call invalidated the retained forward
        eng.stage_backward(torch.zeros(2, 19, 8, 8, device="cuda"), torch.zeros(2, 38, 8, 8, device="cuda"), torch.ones(2, 8, 8, device="cuda"))


def test_state_dict_keeps_the_trained_cpm_after_the_scope_narrows():
    """cpm-scope steps, reset, scope "stages": net.state_dict() still holds the cpm parameters the engine trained, before and
    after further stage-scope steps, and an engine rebuilt from that dict computes what the trained engine computes."""
    net, sd, x, labels, full = make_net("d")
    opt = optim.StageAdam(net, base_lr=oc.LOOP_LR, scope=_lib.TRAIN_CPM)
    assert opt.scope == "cpm" and net.engine.train_scope == "cpm"
    for _ in range(2):
        val.train_step(net, opt, x, labels, full)
    eng = net.engine
    trained = {k: v.cpu().clone() for k, v in eng.stage_params().items()}
    assert list(trained) == cc.grad_keys(sd) and all(not torch.equal(trained[k].reshape(sd[k].shape), sd[k]) for k in trained)
    eng.load_adam_state(None)
    opt2 = optim.StageAdam(net, base_lr=oc.LOOP_LR)                        # narrows the scope to "stages"
    assert eng.train_scope == "stages" and list(eng.stage_params()) == bc.grad_keys(sd)
    got = net.state_dict()
    for k in trained:
        assert torch.equal(got[k].cpu(), trained[k].reshape(sd[k].shape)), k
    val.train_step(net, opt2, x, labels, full)
    got = net.state_dict()
    cur = {k: v.cpu() for k, v in eng.stage_params().items()}
    for k in cc.cpm_keys(sd):
        assert torch.equal(got[k].cpu(), trained[k].reshape(sd[k].shape)), k       # the stage-scope step left the cpm alone
    for k in cur:
        assert torch.equal(got[k].cpu(), cur[k].reshape(sd[k].shape)) and not torch.equal(cur[k], trained[k]), k
    xc = torch.from_numpy(x).cuda()
    want = eng.forward(xc)
    net.load_state_dict(got)                                               # marks the engine for a reload from the net's own copy
    for a, b in zip(net(xc), want):
        assert torch.equal(a, b)


def make_net(name):
    c, NH, NP, sd, x = inputs(name)
    net = PoseEstimationWithMobileNet(num_refinement_stages=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    K = tc.skeleton(c["skel"])[0]
    kp, n = bc.persons(c)
    labels = tc.frames_to_labels([[kp[f, i] for i in range(n[f])] for f in range(c["N"])], K)
    full = np.repeat(np.repeat(bc.loss_mask(c), 8, 1), 8, 2)
    return net, sd, x, labels, full


def test_twenty_steps_in_cpm_scope_lower_the_loss_of_case_d():
    net, sd, x, labels, full = make_net("d")
    opt = optim.StageAdam(net, base_lr=oc.LOOP_LR, weight_decay=oc.WEIGHT_DECAY, scope="cpm")
    assert net.engine.train_scope == "cpm"
    losses = [sum(val.train_step(net, opt, x, labels, full)) for _ in range(oc.LOOP_STEPS)]
    losses.append(sum(val.stage_losses(net, x, labels, full)))
    print("cpm scope, case d: loss %.9g -> %.9g" % (losses[0], losses[-1]))
    assert opt.steps == oc.LOOP_STEPS
    assert losses[-1] < losses[0]
    after = net.state_dict()
    for k in sd:
        if k.startswith("cpm."):
            assert not torch.equal(after[k].cpu(), sd[k]), k
        if k.startswith("model."):
            assert torch.equal(after[k].cpu(), sd[k]), k
    ck = opt.state_dict()
    assert ck["step"] == oc.LOOP_STEPS and list(ck["exp_avg"]) == cc.grad_keys(sd)
    with pytest.raises(Exception):
        net.train(True)
