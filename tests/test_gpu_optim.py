"""Stage fine-tuning step on the GPU (-m gpu): lwp_stage_adam_step's two kernels, its ordering and checkpoints, and the loop
train_forward -> stage_backward -> step of val.train_step, against the float64 restatement of tests/optim_cases.py and against
lwp_load_weights' own host packing.

Bars.  The Adam kernel computes in float64 and rounds each store once, and so does ``adam_ref`` followed by a float32 cast: the
bar is 1 float32 ulp per element (0 unless pow / sqrt / division of the two double libraries differ in the last bit).  The
repacked blob must equal, byte for byte, the blob lwp_load_weights packs from the same raw values.  The loop of case d must
lower the loss by at least half of the drop of the pinned float64 loop; its step-0 loss is held to the pinned float64 value
within tests/test_gpu_train.py's bound for an fp32 quantity against float64, (n + 8) 2^-24 relative, n the elements summed."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, optim, synth, val
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import backward_cases as bc
import optim_cases as oc
import train_cases as tc

pytestmark = pytest.mark.gpu
BASE_LR = 4e-5            # the reference's default (train.py --base-lr)


def make_engine(name, sd=None):
    c, NH, NP, sd0, x = oc.case_state(name)
    eng = Engine(0, nref=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    K, lk, lp = tc.skeleton(c["skel"])
    if c["skel"] != "coco":
        eng.set_skeleton(lk, lp, K)
    eng.load_state_dict(sd0 if sd is None else sd)
    return eng, c, sd0, x


def blob_of(eng):
    t = torch.empty(eng.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    eng.export_weights(t)
    torch.cuda.synchronize()                     # the export's device-to-device copy runs on the null stream, .cpu() on the current one
    return t.cpu().numpy()


def merged(sd, params):
    out = dict(sd)
    out.update({k: v.detach().cpu().reshape(sd[k].shape) for k, v in params.items()})
    return out


# ------------------------------------------------------------------------------------------ 1. the Adam kernel alone
@pytest.mark.parametrize("name", ["a", "e"])
def test_adam_kernel_within_one_ulp_of_float64(name):
    eng, c, sd, _ = make_engine(name)
    spec, total = eng.grad_spec()
    lr, decay = oc.flat_groups(spec, BASE_LR)
    worst, differing, torch_differing, torch_worst = 0, 0, 0, 0
    k0, shape0, off0 = spec[0]
    k1, shape1, off1 = spec[1]
    assert oc.group_of(k0)[1] and not oc.group_of(k1)[1]            # a conv weight (decay on) and its bias (decay off)
    n0, n1 = int(np.prod(shape0)), int(np.prod(shape1))
    first = eng.flat_of(eng.stage_params()).cpu().numpy()
    for t in range(1, 4):
        p0 = eng.flat_of(eng.stage_params()).cpu().numpy()
        st = eng.adam_state()
        assert st["step"] == t - 1
        m0, v0 = st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy()
        g = oc.crafted_gradients(spec, t)
        eng.adam_step(torch.from_numpy(g).cuda(), BASE_LR, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
        p1 = eng.flat_of(eng.stage_params()).cpu().numpy()
        st = eng.adam_state()
        assert st["step"] == t
        got = (p1, st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
        want = oc.adam_ref(p0, g, m0, v0, t, lr, decay)
        for a, w in zip(got, want):
            assert np.isfinite(a).all()
            d = oc.ulp_distance(a, w.astype(np.float32))
            worst = max(worst, int(d.max()))
            differing += int((d != 0).sum())
        # for information: torch's fp32 CPU Adam from the same state
        groups = []
        params = []
        for k, shape, off in spec:
            q = torch.nn.Parameter(torch.from_numpy(p0[off:off + int(np.prod(shape))].copy()))
            q.grad = torch.from_numpy(g[off:off + int(np.prod(shape))].copy())
            mult, wd = oc.group_of(k)
            groups.append({"params": [q], "lr": BASE_LR * mult, "weight_decay": oc.WEIGHT_DECAY if wd else 0})
            params.append((q, off))
        opt = torch.optim.Adam(groups, lr=BASE_LR, betas=oc.BETAS, eps=oc.EPS)
        for q, off in params:
            opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m0[off:off + q.numel()].copy()),
                            "exp_avg_sq": torch.from_numpy(v0[off:off + q.numel()].copy())}
        opt.step()
        tflat = np.concatenate([q.detach().numpy() for q, _ in params])
        d = oc.ulp_distance(tflat, want[0].astype(np.float32))
        torch_differing += int((d != 0).sum())
        torch_worst = max(torch_worst, int(d.max()))
        if t == 1:
            zero_g = g[off0:off0 + n0] == 0
            assert zero_g.any() and (p1[off0:off0 + n0][zero_g] != p0[off0:off0 + n0][zero_g]).any()     # decay alone moves a weight
    print("case %s: %d elements x 3 arrays x 3 steps, worst %d ulp, %d not identical; torch fp32 CPU Adam parameters: worst %d ulp, %d not identical"
          % (name, total, worst, differing, torch_worst, torch_differing))
    last = eng.flat_of(eng.stage_params()).cpu().numpy()
    assert np.array_equal(last[off1:off1 + n1], first[off1:off1 + n1])    # decay off, gradient zero: not one bit moves
    assert worst <= 1


# ------------------------------------------------------------------------------------------ 2. repack, 3. ordering
_steps = {}


def stepped(name):
    """Case engine after one step that was IMMEDIATELY followed by a forward (no synchronise), with the fresh engine that was
    given the same values through lwp_load_weights."""
    if name in _steps:
        return _steps[name]
    eng, c, sd, x = make_engine(name)
    xc = torch.from_numpy(x).cuda()
    before = blob_of(eng)
    eng.forward(xc)
    total = eng.grad_spec()[1]
    g = torch.from_numpy(np.random.RandomState(c["seed"]).standard_normal(total).astype(np.float32)).cuda()
    torch.cuda.synchronize()
    eng.adam_step(g, 1e-2, oc.BETAS, oc.EPS, oc.WEIGHT_DECAY)
    outs = eng.forward(xc)
    params = eng.stage_params()
    fresh, _, _, _ = make_engine(name, merged(sd, params))
    r = dict(eng=eng, fresh=fresh, sd=sd, xc=xc, before=before, outs=outs, params=params, c=c)
    _steps[name] = r
    return r


@pytest.mark.parametrize("name", ["a", "b", "d", "e"])
def test_repacked_blob_is_the_blob_load_weights_packs(name):
    r = stepped(name)
    got, want = blob_of(r["eng"]), blob_of(r["fresh"])
    assert got.shape == want.shape == r["before"].shape
    assert not np.array_equal(got, r["before"])
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "first differing byte %d of %d" % (diff[0], got.size)
    for k, v in r["params"].items():                                   # the step moved every stage parameter
        assert not torch.equal(v.cpu().reshape(r["sd"][k].shape), r["sd"][k]), k


@pytest.mark.parametrize("name", ["a", "e"])
def test_forward_right_after_the_step_sees_the_new_weights(name):
    r = stepped(name)
    want = r["fresh"].forward(r["xc"])
    assert len(want) == len(r["outs"]) == 2 * (r["c"]["nref"] + 1)
    for a, b in zip(r["outs"], want):
        assert torch.equal(a, b)


def test_step_invalidates_the_retained_forward_and_refuses_other_handles():
    eng, c, sd, x = make_engine("a")
    xc = torch.from_numpy(x).cuda()
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (c["H"], c["W"]))
    mask = torch.from_numpy(bc.loss_mask(c)).cuda()
    eng.train_forward(xc)
    grads, _ = eng.stage_backward(km, pm, mask)
    flat = eng.flat_of(grads)
    eng.adam_step(flat, BASE_LR)
    with pytest.raises(ValueError, match="lwp_train_forward"):
        eng.stage_backward(km, pm, mask)
    eng.train_forward(xc)
    eng.stage_backward(km, pm, mask)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="base_lr"):
            eng.adam_step(flat, bad)
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, float("nan"))):
        with pytest.raises(ValueError, match="betas"):
            eng.adam_step(flat, BASE_LR, betas)
    with pytest.raises(ValueError, match="gradient-spec"):
        eng.adam_step(flat[:-1], BASE_LR)
    # a handle whose weights came from a blob has no raw parameters
    twin = Engine(0, nref=c["nref"], num_channels=c["C"])
    blob = torch.empty(eng.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    eng.export_weights(blob)
    twin.import_weights(blob)
    with pytest.raises(ValueError, match="raw parameters"):
        twin.adam_step(flat, BASE_LR)
    with pytest.raises(ValueError, match="raw parameters"):
        twin.stage_params()
    half = Engine(0, nref=1, num_channels=64, dtype=_lib.BF16)
    half.load_state_dict(synth.make_state_dict(1, seed=1, num_channels=64))
    f64 = torch.zeros(half.grad_spec()[1], device="cuda")
    with pytest.raises(ValueError, match="fp32"):
        half.adam_step(f64, BASE_LR)
    h16 = Engine(0, nref=1, num_channels=64, dtype=_lib.F16)
    h16.load_state_dict(synth.make_state_dict(1, seed=1, num_channels=64))
    with pytest.raises(ValueError, match="fp32"):
        h16.adam_step(f64, BASE_LR)
    # pending work
    eng.pipeline_submit(xc, 0)
    with pytest.raises(RuntimeError, match="pending"):
        eng.adam_step(flat, BASE_LR)
    eng.pipeline_fetch(0)
    eng.infer_poses_async(xc)
    with pytest.raises(RuntimeError, match="pending"):
        eng.adam_step(flat, BASE_LR)
    eng.fetch_poses()
    eng.adam_step(flat, BASE_LR)


def test_export_and_load_right_after_a_step_on_a_side_stream():
    """The blob copies of export / import / load are host-synchronous copies, not stream work: they wait for a queued step."""
    eng, c, sd, x = make_engine("a")
    total = eng.grad_spec()[1]
    g = torch.from_numpy(np.random.RandomState(3).standard_normal(total).astype(np.float32)).cuda()
    junk = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            junk = (junk @ junk) * 1e-3                  # the step waits behind this on the caller's stream
        eng.adam_step(g, 1e-2)
        got = blob_of(eng)                               # no synchronise in between
    fresh, _, _, _ = make_engine("a", merged(sd, eng.stage_params()))
    assert np.array_equal(got, blob_of(fresh))
    assert not np.array_equal(got, blob_of(make_engine("a")[0]))
    # a load queued right behind a step wins: the repack does not overwrite it
    with torch.cuda.stream(side):
        for _ in range(40):
            junk = (junk @ junk) * 1e-3
        eng.adam_step(g, 1e-2)
        eng.load_state_dict(sd)
    side.synchronize()
    assert np.array_equal(blob_of(eng), blob_of(make_engine("a")[0]))
    # a direct Engine.adam_step on a net's engine is seen by net.state_dict()
    net, c, sd, x, labels, full = make_net("d")
    before = net.state_dict()
    net.engine.adam_step(torch.ones(net.engine.grad_spec()[1], device="cuda"), 1e-2)
    after = net.state_dict()
    assert all(not torch.equal(after[k], before[k]) for k in bc.grad_keys(sd))


# ------------------------------------------------------------------------------------------ 4. determinism and checkpoint
def make_net(name):
    c, NH, NP, sd, x = oc.case_state(name)
    net = PoseEstimationWithMobileNet(num_refinement_stages=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    K, lk, lp = tc.skeleton(c["skel"])
    if c["skel"] != "coco":
        net.engine.set_skeleton(lk, lp, K)
    kp, n = bc.persons(c)
    labels = tc.frames_to_labels([[kp[f, i] for i in range(n[f])] for f in range(c["N"])], K)
    full = np.repeat(np.repeat(bc.loss_mask(c), 8, 1), 8, 2)
    return net, c, sd, x, labels, full


def test_two_engines_agree_and_a_checkpoint_resumes_bit_for_bit():
    nets = [make_net("b") for _ in range(2)]
    opts = [optim.StageAdam(n[0], base_lr=1e-3) for n in nets]
    for _ in range(2):
        for (net, c, sd, x, labels, full), opt in zip(nets, opts):
            val.train_step(net, opt, x, labels, full)
    b0, b1 = blob_of(nets[0][0].engine), blob_of(nets[1][0].engine)
    assert np.array_equal(b0, b1)
    s0, s1 = nets[0][0].engine.adam_state(), nets[1][0].engine.adam_state()
    assert s0["step"] == s1["step"] == 2
    assert torch.equal(s0["exp_avg"], s1["exp_avg"]) and torch.equal(s0["exp_avg_sq"], s1["exp_avg_sq"])
    # checkpoint of the first net into a third
    net0, c, sd, x, labels, full = nets[0]
    ck_net, ck_opt = net0.state_dict(), opts[0].state_dict()
    assert ck_opt["step"] == 2 and set(ck_opt["exp_avg"]) == set(bc.grad_keys(sd)) == set(ck_opt["exp_avg_sq"])
    assert any(not torch.equal(ck_net[k], sd[k]) for k in bc.grad_keys(sd))
    assert all(torch.equal(ck_net[k], sd[k]) for k in sd if k not in bc.grad_keys(sd))      # nothing else moved
    net3 = make_net("b")[0]
    net3.load_state_dict(ck_net)
    opt3 = optim.StageAdam(net3, base_lr=1e-3)
    opt3.load_state_dict(ck_opt)
    net3.cuda()
    assert np.array_equal(blob_of(net3.engine), b0)                     # the saved dict gives the same blob
    l0 = val.train_step(net0, opts[0], x, labels, full)
    l3 = val.train_step(net3, opt3, x, labels, full)
    assert l0 == l3
    assert np.array_equal(blob_of(net3.engine), blob_of(net0.engine))
    a, b = net0.engine.stage_params(), net3.engine.stage_params()
    assert torch.equal(net0.engine.flat_of(a), net3.engine.flat_of(b))
    s0, s3 = net0.engine.adam_state(), net3.engine.adam_state()
    assert s0["step"] == s3["step"] == 3 and torch.equal(s0["exp_avg"], s3["exp_avg"]) and torch.equal(s0["exp_avg_sq"], s3["exp_avg_sq"])


# ------------------------------------------------------------------------------------------ 5. accumulation
def test_train_step_accumulates_two_batches_into_one_step():
    net, c, sd, x, labels, full = make_net("a")
    opt = optim.StageAdam(net, base_lr=1e-3)
    start = blob_of(net.engine)
    ones = np.ones_like(full)
    val.train_step(net, opt, x, labels, full, batches_per_iter=2)
    assert opt.steps == 0 and np.array_equal(blob_of(net.engine), start)
    val.train_step(net, opt, x, labels, ones, batches_per_iter=2)
    assert opt.steps == 1 and opt.batch_index == 0
    # the same by hand on a second engine: the sum of two backward passes at loss_scale 1 / 2, one step
    eng, _, _, _ = make_engine("a")
    xc = torch.from_numpy(x).cuda()
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (c["H"], c["W"]))
    eng.train_forward(xc)
    g, _ = eng.stage_backward(km, pm, torch.from_numpy(bc.loss_mask(c)).cuda(), loss_scale=0.5)
    flat = eng.flat_of(g)
    eng.train_forward(xc)
    eng.stage_backward(km, pm, torch.ones(c["N"], c["H"] // 8, c["W"] // 8, device="cuda"), loss_scale=0.5, into=flat)
    eng.adam_step(flat, 1e-3)
    assert np.array_equal(blob_of(net.engine), blob_of(eng))
    assert not np.array_equal(blob_of(eng), start)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.train(True)


# ------------------------------------------------------------------------------------------ 6. the loop
def test_twenty_steps_lower_the_loss_of_case_d():
    net, c, sd, x, labels, full = make_net("d")
    opt = optim.StageAdam(net, base_lr=oc.LOOP_LR, weight_decay=oc.WEIGHT_DECAY)
    losses = [sum(val.train_step(net, opt, x, labels, full)) for _ in range(oc.LOOP_STEPS)]
    losses.append(sum(val.stage_losses(net, x, labels, full)))
    n = (c["nref"] + 1) * c["N"] * sum(bc.channels(c)) * (c["H"] // 8) * (c["W"] // 8)
    print("loss %.9g -> %.9g (float64 loop: %.9g -> %.9g); step-0 difference %.3g, bound %.3g"
          % (losses[0], losses[-1], oc.LOOP_LOSS0, oc.LOOP_LOSS20, abs(losses[0] - oc.LOOP_LOSS0), (n + 8) * 2.0 ** -24 * losses[0]))
    assert opt.steps == oc.LOOP_STEPS
    assert abs(losses[0] - oc.LOOP_LOSS0) <= (n + 8) * 2.0 ** -24 * losses[0]
    assert losses[0] - losses[-1] >= 0.5 * (oc.LOOP_LOSS0 - oc.LOOP_LOSS20)
