"""The backward's 16-bit mode on the GPU (-m gpu): lwp_set_backward_precision, dgrad_h16_kernel / wgrad_h16_kernel alone through
lwp_debug_conv_grad on the fixtures of tests/backward_h16_cases.py, and end to end in the three train scopes.

Integer fixtures: no operand rounds (|dz| S <= 512, |x|, |w| <= 8) and every scaled product and partial sum is an integer below
2^24 (tests/test_backward_h16_host.py checks both), so dx, dw and db equal the int64 statement on every element, whatever the K
order, the MFMA shape or the split count.
Normal fixtures, per element: |got - want64_h16| <= (depth + 8) 2^-23 sum|terms_h16|, want64_h16 the float64 statement on the
operands rounded as the kernels round them.  The constant is twice the f32 kernels': the f32 MFMA is a k-ordered fmaf chain, one
rounding of 2^-24 per product; how a 16x16x32 MFMA adds its 32 exact products is not documented, and either plausible scheme,
a truncating add (2^-23 per add) or an alignment to the largest term with at least 24 bits kept (2^-23 of that term per term),
fits under 2^-23 per term.  The test prints the worst error / bound per shape and mode (-s); DESIGN.md section 3q has the figures.
db is fp32 mode's db bit for bit.
Measured on the MI355X: every case lies under the bound, bf16 at most 0.042, fp16 at most 0.047.  (A first form of the fp16
kernels missed it on [3x2x3x57x132x3x2xgraph-fp16-scale1], dw at 1.65: with a subnormal fp16 operand the MFMA aligns its addends
to the nominal exponent 2^-14 and keeps 24 bits below that.  The kernels now split such operands off)
End to end: e(g) = max|g - g64| / max|g64| per tensor against the float64 restatement on the device's own branch masks;
the bar of every tensor is e <= 2 e_sim + 8 e_ref: e_sim the largest e over the tensors of the float64 restatement that rounds
dZ S, x and the folded w where the kernels do (the error the format itself costs; one figure per case, as e_ref is), 8 e_ref the
fp32 bar for the accumulation, the factor 2 for the operands whose 16-bit rounding flips because the retained f32 activation
differs from the float64 one in its last bits.  In scope "all" the restatement's forward starts at the image, its activations
differ from the device's by the whole backbone's f32 error, and the two sets of roundings decorrelate on the way down: a single
tensor's e then reaches 3.2 times that tensor's own restated error (printed), while staying inside the case's bar."""
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
import backward_h16_cases as hc
import backward_kernel_cases as kc
import cpm_backward_cases as cc
import optim_cases as oc
import train_cases as tc

pytestmark = pytest.mark.gpu
S = kc.SENTINEL
_eng = []
_fp32_db = {}
ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]
mode_ids = ["%s-scale%g" % m for m in hc.MODES]


def engine():
    if not _eng:
        _eng.append(Engine(0, nref=1))
    return _eng[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def run_dense(eng, shape, t, chunk, acc_from, no_bias, accumulate, windows=None):
    """dx, dw, db of one lwp_debug_conv_grad call in the engine's current precision; the split count, the guard rows and the
    window margins checked."""
    N, H, W, cout, cin, ks, dil, mode = shape
    dx, dw, db, splits, rows = eng.debug_conv_grad(t["dz"], t["x"], t["w"], dil=dil, pad=mode, max_chunk=chunk, acc_from=acc_from, no_bias=no_bias,
                                                   accumulate=accumulate, dx0=t["dx0"], dw0=t["dw0"], db0=t["db0"], windows=windows, fill=S)
    M = kc.dense_M(shape)
    if chunk:
        assert splits == (M + chunk - 1) // chunk
    else:
        assert 1 <= splits <= (M + 63) // 64
    lo = windows[2][1] if windows else 0
    r = host(rows)
    assert r.shape[0] == M + Engine.GUARD_ROWS and (r[M:] == S).all() and (r[:M, :lo] == S).all() and (r[:M, lo + cin:] == S).all(), \
        (shape, chunk, acc_from, no_bias, accumulate, windows)
    return dict(dx=host(dx), dw=host(dw), db=host(db))


def cases_of(shape):
    """(acc_from, no_bias, accumulate, windows): every flag combination in plain rows, one of them in the merged heads' windows."""
    cout, cin = shape[3], shape[4]
    (zp, zo), (xp, xo), (dp, do) = kc.WINDOWS
    win = ((cout + zp, zo), (cin + xp, xo), (cin + dp, do))
    flags = [(a, nb, acc, None) for a in kc.acc_from_values(cin) for nb in (0, 1) for acc in (0, 1)]
    return flags + [(kc.acc_from_values(cin)[-1], 0, 1, win)]


def set_mode(eng, precision, scale):
    eng.set_backward_precision(precision, scale)
    assert eng.backward_precision == (precision, scale)


# ---------------------------------------------------------------------------------------------- 1. integer fixtures
@pytest.mark.parametrize("mode", hc.MODES, ids=mode_ids)
@pytest.mark.parametrize("shape", hc.DENSE_SHAPES, ids=ids(hc.DENSE_SHAPES))
def test_integer_fixtures_bit_for_bit(shape, mode):
    f = kc.dense_fixture(shape, "int")
    t = dict((k, dev(v)) for k, v in f.items())
    eng = engine()
    set_mode(eng, *mode)
    try:
        for a, nb, acc, win in cases_of(shape):
            want, _ = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, nb, acc)
            for chunk in hc.CHUNKS:
                assert kc.exact_failures(run_dense(eng, shape, t, chunk, a, nb, acc, win), want) == [], (shape, mode, chunk, a, nb, acc, win)
    finally:
        eng.set_backward_precision("fp32", 1.0)


# ---------------------------------------------------------------------------------------------- 2. normal fixtures
def fp32_db(shape, t, chunk, a, nb, acc, win):
    """db of the f32 kernels for the same call (the engine is left in fp32 mode), computed once per call signature."""
    key = (shape, chunk, a, nb, acc, win)
    if key not in _fp32_db:
        eng = engine()
        eng.set_backward_precision("fp32", 1.0)
        _fp32_db[key] = run_dense(eng, shape, t, chunk, a, nb, acc, win)["db"]
    return _fp32_db[key]


@pytest.mark.parametrize("mode", hc.MODES, ids=mode_ids)
@pytest.mark.parametrize("shape", hc.DENSE_SHAPES, ids=ids(hc.DENSE_SHAPES))
def test_normal_fixtures_per_element(shape, mode):
    f32 = kc.dense_fixture(shape, "normal")
    t = dict((k, dev(v)) for k, v in f32.items())
    eng = engine()
    worst = dict(dx=0.0, dw=0.0, db=0.0)
    over = []
    try:
        for a, nb, acc, win in cases_of(shape):
            want, terms = hc.dense_results_h16(f32["dz"], f32["x"], f32["w"], shape[6], f32["dx0"], f32["dw0"], f32["db0"], a, nb, acc, *mode)
            depths = kc.dense_depths(shape, a, acc)
            for chunk in hc.CHUNKS:
                db32 = fp32_db(shape, t, chunk, a, nb, acc, win)
                set_mode(eng, *mode)
                got = run_dense(eng, shape, t, chunk, a, nb, acc, win)
                r = hc.bound_ratios_h16(got, want, terms, depths)
                worst = dict((k, max(worst[k], r[k])) for k in r)
                assert np.array_equal(got["db"].view(np.uint32), db32.view(np.uint32)), (shape, mode, chunk, a, nb, acc, win)
                over += [(chunk, a, nb, acc, win, k, r[k]) for k in r if not r[k] <= 1.0]
    finally:
        eng.set_backward_precision("fp32", 1.0)
        print("dgrad_h16 / wgrad_h16 + reduce / bias %s %s scale %g: worst error / bound %s" %
              (shape, mode[0], mode[1], ", ".join("%s %.3g" % (k, v) for k, v in sorted(worst.items()))))
    assert over == [], (shape, mode, over)


# ---------------------------------------------------------------------------------------------- 3. switching
@pytest.mark.parametrize("shape", [hc.DENSE_SHAPES[3], hc.DENSE_SHAPES[7]], ids=ids([hc.DENSE_SHAPES[3], hc.DENSE_SHAPES[7]]))
def test_fp32_after_bf16_is_a_fresh_handles_fp32_and_bf16_repeats_itself(shape):
    f32 = kc.dense_fixture(shape, "normal")
    t = dict((k, dev(v)) for k, v in f32.items())
    a, nb, acc, win = cases_of(shape)[-1]
    eng, fresh = engine(), Engine(0, nref=1)
    assert fresh.backward_precision == ("fp32", 1.0)
    for chunk in hc.CHUNKS:
        set_mode(eng, "bf16", 1.0)
        first = run_dense(eng, shape, t, chunk, a, nb, acc, win)
        second = run_dense(eng, shape, t, chunk, a, nb, acc, win)
        set_mode(eng, "fp32", 1.0)
        back = run_dense(eng, shape, t, chunk, a, nb, acc, win)
        want = run_dense(fresh, shape, t, chunk, a, nb, acc, win)
        for k in first:
            assert np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)), (k, chunk)
            assert np.array_equal(back[k].view(np.uint32), want[k].view(np.uint32)), (k, chunk)
        assert not np.array_equal(first["dx"], back["dx"]) and not np.array_equal(first["dw"], back["dw"])      # the mode did switch


# ---------------------------------------------------------------------------------------------- 4. end to end
_e2e = {}


def e2e(scope):
    """Engine in ``scope`` behind a retaining forward of the scope's smallest case, the float64 references on the device's own
    masks and the fp32 CPU reference error, computed once."""
    if scope in _e2e:
        return _e2e[scope]
    cases, name = hc.E2E_CASES[scope]
    c = cases[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    eng = Engine(0, nref=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    K, lk, lp = tc.skeleton(c["skel"])
    if c["skel"] != "coco":
        eng.set_skeleton(lk, lp, K)
    eng.set_train_scope(scope)
    eng.load_state_dict(sd)
    xc = torch.from_numpy(x).cuda()
    hs, ws = bb.map_dims(c)
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (8 * hs, 8 * ws))
    mask = torch.from_numpy(bb.loss_mask(c)).cuda()
    eng.train_forward(xc)
    layers = eng.layers()
    first = [i["index"] for i in layers if i["name"] == "cpm.conv"][0]
    acts = {i["index"]: eng.train_activation(i["index"]) for i in layers if i["index"] >= first}
    masks = cc.stage_masks(layers, acts)
    start = torch.from_numpy(acts[first])
    if scope != "stages":
        cacts = eng.cpm_activations()
        masks["cpm.align"] = torch.from_numpy(cacts["cpm.align"]) > 0
        masks["cpm.conv"] = torch.from_numpy(cacts["cpm"]) > 0
        start = torch.from_numpy(cacts["model.11"])
    if scope == "all":
        bacts = eng.backbone_activations()
        for nm in bb.RELU_LAYERS:
            masks[nm] = torch.from_numpy(bacts[nm]) > 0
        start = torch.from_numpy(x)
    args = (sd, start, c["nref"], km.cpu(), pm.cpu(), mask.cpu(), c["N"])
    grad = hc.GRADIENTS[scope]
    g64, taps64 = grad(*args, masks=masks)[:2]
    bc.check_mask_deviation(masks, taps64)
    g32, taps32 = grad(*args, dtype=torch.float32)[:2]
    g64_32 = grad(*args, masks=bc.own_masks(taps32))[0]
    e_ref = max(bc.err(g32[k], g64_32[k]) for k in g64_32)
    _, stats = hc.sim_gradients(scope, "fp32", 1.0, *args, masks=masks)
    r = dict(name=name, c=c, eng=eng, km=km, pm=pm, mask=mask, args=args, masks=masks, g64=g64, e_ref=e_ref, max_dz=stats["max_dz"])
    _e2e[scope] = r
    return r


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("scope", ["stages", "cpm", "all"])
def test_gradients_against_float64_within_twice_the_formats_own_error(scope, precision):
    r = e2e(scope)
    eng = r["eng"]
    scale = 1.0 if precision == "bf16" else hc.fp16_scale(r["max_dz"])
    sim, stats = hc.sim_gradients(scope, precision, scale, *r["args"], masks=r["masks"])
    set_mode(eng, precision, scale)
    try:
        out = eng.stage_backward(r["km"], r["pm"], r["mask"], want_backbone=scope != "stages")
        torch.cuda.synchronize()
    finally:
        eng.set_backward_precision("fp32", 1.0)
    got = dict(out[0], d_features=out[1])
    if scope != "stages":
        got["d_backbone"] = out[2]
    assert set(got) == set(r["g64"])
    # e_sim is one figure per case, the largest over the tensors, as e_ref is; every tensor is held to the case's bar
    e_sim = max(bc.err(sim[k], r["g64"][k]) for k in got)
    e = dict((k, bc.err(got[k].cpu(), r["g64"][k])) for k in got)
    worst = max(e, key=e.get)
    per_tensor = max(e[k] / max(bc.err(sim[k], r["g64"][k]), 8 * r["e_ref"]) for k in got)
    failed = [(k, e[k]) for k in sorted(got) if not e[k] <= 2 * e_sim + 8 * r["e_ref"]]
    print("scope %s case %s %s scale %g: e %.3g (%s), e_sim %.3g, e_ref %.3g; largest e / its own tensor's e_sim %.3g; %d of %d non-zero dz round to zero" %
          (scope, r["name"], precision, scale, e[worst], worst, e_sim, r["e_ref"], per_tensor, stats["flushed"], stats["nonzero"]))
    assert failed == [], (r["e_ref"], failed)


# ---------------------------------------------------------------------------------------------- 5. stale weights
def make_net(c, sd):
    NH, NP = bc.channels(c)
    net = PoseEstimationWithMobileNet(num_refinement_stages=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    return net


def test_the_backward_after_a_step_reads_the_new_weights():
    """One bf16 train_step in scope "all" (stage convs, the cpm's 1x1s and the backbone's folded pointwise matrices all change),
    then a gradient: an engine built from the stepped parameters gives the same bits, so nothing 16-bit was kept from before."""
    c = bc.CASES["d"]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    kp, n = bc.persons(c)
    labels = tc.frames_to_labels([[kp[f, i] for i in range(n[f])] for f in range(c["N"])], tc.skeleton(c["skel"])[0])
    full = np.repeat(np.repeat(bc.loss_mask(c), 8, 1), 8, 2)
    net = make_net(c, sd)
    opt = optim.StageAdam(net, base_lr=oc.LOOP_LR, scope="all", backward_precision="bf16")
    assert net.engine.backward_precision == ("bf16", 1.0)
    before = val.stage_gradients(net, x, labels, full)[1]
    before = net.engine.flat_of(before).clone()
    val.train_step(net, opt, x, labels, full)
    _, grads, dfeat = val.stage_gradients(net, x, labels, full)
    flat = net.engine.flat_of(grads)
    assert not torch.equal(flat, before)                                   # the step moved the weights the backward reads
    fresh = make_net(c, net.state_dict())
    optim.StageAdam(fresh, base_lr=oc.LOOP_LR, scope="all", backward_precision="bf16", grad_scale=1.0)
    _, grads2, dfeat2 = val.stage_gradients(fresh, x, labels, full)
    assert torch.equal(fresh.engine.flat_of(grads2), flat) and torch.equal(dfeat2, dfeat)


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_broken_argument_rules_are_refused_and_leave_the_setting_alone():
    eng = engine()
    eng.set_backward_precision("fp32", 1.0)
    L = _lib.lib()
    for dtype, scale in ((_lib.BF16, 3.0), (_lib.F16, 0.5), (_lib.F32, 2.0), (7, 1.0), (_lib.BF16, 2.0 ** 25), (_lib.BF16, float("nan"))):
        assert L.lwp_set_backward_precision(eng.h.ptr, dtype, scale) == _lib.LWP_ERR_ARG, (dtype, scale)
        assert L.lwp_last_error(eng.h.ptr)
        assert eng.backward_precision == ("fp32", 1.0)
    with pytest.raises(ValueError, match="power of two"):
        eng.set_backward_precision("bf16", 3)
    with pytest.raises(ValueError, match="power of two"):
        eng.set_backward_precision("fp16", 0.5)
    with pytest.raises(ValueError, match="must be 1"):
        eng.set_backward_precision("fp32", 2)
    with pytest.raises(ValueError, match="backward precision"):
        eng.set_backward_precision("fp8", 1)
    for dtype in (_lib.BF16, _lib.F16):
        half = Engine(0, nref=1, num_channels=64, dtype=dtype)
        with pytest.raises(ValueError, match="fp32 handles only"):
            half.set_backward_precision("bf16", 1.0)
    eng.set_backward_precision("fp16", 2.0 ** 24)
    assert eng.backward_precision == ("fp16", 2.0 ** 24)
    eng.set_backward_precision()
    assert eng.backward_precision == ("fp32", 1.0)
