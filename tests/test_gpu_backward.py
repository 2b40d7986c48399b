"""Stage backward on the GPU (-m gpu): lwp_train_forward / lwp_stage_backward against the float64 restatement of
tests/backward_cases.py, which differentiates the branch the device took (its ReLU masks come from the retained activations,
within backward_cases' cap) starting from the device's own cpm output.

The bar of a gradient tensor g is e(g) = max|g - g64| / max|g64| <= 8 e_ref, e_ref being the largest e of torch's fp32 CPU
autograd over the same restatement on the same inputs against float64 on the fp32 run's own masks."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth, val
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine
from lwpose_amd import _lib
from oracle import net_ref

import backward_cases as bc
import train_cases as tc

pytestmark = pytest.mark.gpu
NET_TOL = 1e-3            # the per-layer parity bound of tests/test_gpu_parity.py
_runs = {}


def inputs(name):
    c = bc.CASES[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    return c, NH, NP, sd, x


def device_masks(eng, acts):
    masks = {}
    for info in eng.layers():
        nm, a = info["name"], acts.get(info["index"])
        if a is None or nm == "cpm.conv" or nm.endswith(".1") and not nm.endswith(".trunk.1"):
            continue
        a = torch.from_numpy(a)
        if nm.endswith(".heads.0"):
            half = a.shape[1] // 2
            masks[nm[:-len("heads.0")] + "heatmaps.0"] = a[:, :half] > 0
            masks[nm[:-len("heads.0")] + "pafs.0"] = a[:, half:] > 0
        elif nm.startswith("refinement_stages.") and nm.endswith(".trunk.1"):
            ini = [i for i in eng.layers() if i["name"] == nm[:-len(".trunk.1")] + ".initial"][0]
            masks[nm] = a > torch.from_numpy(acts[ini["index"]])      # the retained tensor is relu(z) + initial_features
        else:
            masks[nm] = a > 0
    return masks


def run(name):
    """Engine, device results and both references of a case, computed once."""
    if name in _runs:
        return _runs[name]
    c, NH, NP, sd, x = inputs(name)
    eng = Engine(0, nref=c["nref"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    K, lk, lp = tc.skeleton(c["skel"])
    if c["skel"] != "coco":
        eng.set_skeleton(lk, lp, K)
    eng.load_state_dict(sd)
    xc = torch.from_numpy(x).cuda()
    kp, n = bc.persons(c)
    km, pm = eng.train_targets(kp, n, (c["H"], c["W"]))
    mask = torch.from_numpy(bc.loss_mask(c)).cuda()
    fwd = eng.forward(xc)
    outs = eng.train_forward(xc)
    grads, dfeat = eng.stage_backward(km, pm, mask)
    torch.cuda.synchronize()
    layers = eng.layers()
    first = [i["index"] for i in layers if i["name"] == "cpm.conv"][0]
    acts = {i["index"]: eng.train_activation(i["index"]) for i in layers if i["index"] >= first}
    splits = {i["name"]: eng.backward_splits(i["index"]) for i in layers if i["index"] > first}
    feat = torch.from_numpy(acts[first]).double()
    masks = device_masks(eng, acts)
    args = (sd, feat, c["nref"], km.cpu(), pm.cpu(), mask.cpu(), c["N"])
    g64, taps64, outs64 = bc.gradients(*args, masks=masks)
    g32, taps32, _ = bc.gradients(*args, dtype=torch.float32)
    g64_32, _, _ = bc.gradients(*args, masks=bc.own_masks(taps32))
    e_ref = max(bc.err(g32[k], g64_32[k]) for k in g64_32)
    r = dict(c=c, sd=sd, x=x, xc=xc, eng=eng, km=km, pm=pm, mask=mask, fwd=fwd, outs=outs, grads=grads, dfeat=dfeat, acts=acts,
             splits=splits, first=first, masks=masks, g64=g64, taps64=taps64, outs64=outs64, e_ref=e_ref)
    _runs[name] = r
    return r


CASE_NAMES = ["a", "b", "c", "d", "n8"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_outputs_are_those_of_forward_and_activations_match_the_oracle(name):
    r = run(name)
    c, eng = r["c"], r["eng"]
    assert len(r["outs"]) == 2 * (c["nref"] + 1)
    for a, b in zip(r["outs"], r["fwd"]):
        assert torch.equal(a, b)
    if name != "c":          # the float64 backbone of a 368 x 368 frame takes a minute on the CPU: the small cases pin cpm.conv
        taps = {}
        net_ref.forward64(r["sd"], torch.from_numpy(r["x"]), c["nref"], taps, stop_after="cpm")
        ref = taps["cpm"].numpy()
        assert np.abs(r["acts"][r["first"]] - ref).max() <= NET_TOL * max(1.0, np.abs(ref).max())
    # every retained stage layer against the float64 restatement on the device's cpm output
    relu64 = {k: (z * r["masks"][k]).numpy() for k, z in r["taps64"].items()}
    names = {i["index"]: i["name"] for i in eng.layers()}
    checked = 0
    for idx, a in r["acts"].items():
        nm = names[idx]
        if nm.endswith(".heads.0"):
            p = nm[:-len("heads.0")]
            ref = np.concatenate([relu64[p + "heatmaps.0"], relu64[p + "pafs.0"]], 1)
        elif nm.endswith(".heads.1"):
            s = 0 if nm.startswith("initial") else 1 + int(nm.split(".")[1])
            ref = np.concatenate([r["outs64"][2 * s].numpy(), r["outs64"][2 * s + 1].numpy()], 1)
            assert np.array_equal(a, np.concatenate([r["outs"][2 * s].cpu().numpy(), r["outs"][2 * s + 1].cpu().numpy()], 1))
        elif nm.startswith("refinement_stages.") and nm.endswith(".trunk.1"):
            ref = relu64[nm] + relu64[nm[:-len(".trunk.1")] + ".initial"]
        elif nm in relu64:
            ref = relu64[nm]
        else:
            continue
        assert a.shape == ref.shape, nm
        assert np.abs(a - ref).max() <= NET_TOL * max(1.0, np.abs(ref).max()), nm
        checked += 1
    assert checked == 5 + 17 * c["nref"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_against_float64(name):
    r = run(name)
    bc.check_mask_deviation(r["masks"], r["taps64"])
    want = set(bc.grad_keys(r["sd"]))
    assert set(r["grads"]) == want and not any("running_" in k for k in r["grads"])
    worst = 0.0
    got = dict(r["grads"], d_features=r["dfeat"])
    for k in sorted(got):
        assert tuple(got[k].shape) == tuple(r["g64"][k].shape), k       # the merged heads' zero blocks are not part of any tensor
        e = bc.err(got[k].cpu(), r["g64"][k])
        worst = max(worst, e)
        print("case %s %-55s e %.3g" % (name, k, e))
    print("case %s: worst e %.3g, e_ref %.3g, bar %.3g" % (name, worst, r["e_ref"], 8 * r["e_ref"]))
    for k in got:
        assert bc.err(got[k].cpu(), r["g64"][k]) <= 8 * r["e_ref"], k
    if name == "c":
        assert min(r["splits"].values()) > 1, r["splits"]                # more than one pixel range per weight gradient


@pytest.mark.parametrize("name", ["c", "n8"])
def test_rendered_targets_match_the_restatement(name):
    """The targets every side of the comparisons above was handed are the device's own: 46 x 46 maps (nine workgroups a frame)
    in case c, two frames of the guide5 table in n8.  Same bar as tests/test_gpu_train.py: touched sets identical, 1 float32 ulp."""
    r = run(name)
    c = r["c"]
    K, lk, lp = tc.skeleton(c["skel"])
    kp, n = bc.persons(c)
    want = tc.targets(kp, n, c["H"], c["W"], 8, 7, 1, K, tc.limb_rows(lk, lp))
    for what, got, w in (("keypoint_maps", r["km"], want[0]), ("paf_maps", r["pm"], want[1])):
        got = got.cpu().numpy()
        assert got.shape == w.shape and got.dtype == np.float32 and tc.touched(w).any()
        assert np.array_equal(tc.touched(got), tc.touched(w)), (name, what)
        u = tc.ulp_distance(got, w)
        print("case %s %s: %d of %d elements not bit-identical" % (name, what, int((u > 0).sum()), u.size))
        assert u.max() <= 1, (name, what)


def test_losses_of_18_stage_tensors_match_float64():
    """Engine.stage_losses on n8's own outputs: tensors 16 and 17 come from the second loss launch."""
    r = run("n8")
    N = r["c"]["N"]
    assert len(r["outs"]) == 18
    got = r["eng"].stage_losses(r["outs"], r["km"], r["pm"], r["mask"], N)
    assert got == r["eng"].stage_losses(r["outs"], r["km"], r["pm"], r["mask"], N) and len(set(got)) == 18
    km, pm, mask = r["km"].cpu().numpy(), r["pm"].cpu().numpy(), r["mask"].cpu().numpy()
    worst = 0.0
    for i, o in enumerate(r["outs"]):
        o = o.cpu().numpy()
        want = tc.l2_loss64(o, pm if i % 2 else km, mask, N)
        worst = max(worst, abs(got[i] - want) / (o.size * 2.0 ** -52 * want))
        assert got[i] > 0 and abs(got[i] - want) <= o.size * 2.0 ** -52 * want, (i, got[i], want)
    print("case n8: worst loss error %.3g of its bar" % worst)


@pytest.mark.parametrize("name", ["a", "b"])
def test_scale_accumulate_and_determinism(name):
    r = run(name)
    eng, N = r["eng"], r["c"]["N"]
    flat = eng.flat_of(r["grads"]).clone()
    dfeat = r["dfeat"].clone()
    eng.train_forward(r["xc"])
    g, d = eng.stage_backward(r["km"], r["pm"], r["mask"])
    assert torch.equal(eng.flat_of(g), flat) and torch.equal(d, dfeat)                    # same inputs, same bits
    g, d = eng.stage_backward(r["km"], r["pm"], r["mask"], loss_scale=0.25)
    assert torch.equal(eng.flat_of(g), flat * 0.25) and torch.equal(d, dfeat * 0.25)
    g, d = eng.stage_backward(r["km"], r["pm"], r["mask"], batch_size=2 * N)
    assert torch.equal(eng.flat_of(g), flat * 0.5) and torch.equal(d, dfeat * 0.5)
    g2, _ = eng.stage_backward(r["km"], r["pm"], r["mask"], loss_scale=0.25)
    second = eng.flat_of(g2).clone()
    acc = flat.clone()
    eng.stage_backward(r["km"], r["pm"], r["mask"], loss_scale=0.25, into=acc)
    assert torch.equal(acc, flat + second)


def test_argument_checks():
    r = run("a")
    c = r["c"]
    NH, NP = bc.channels(c)
    km, pm, mask = r["km"], r["pm"], r["mask"]
    fresh = Engine(0, nref=1, num_channels=32)
    with pytest.raises(ValueError, match="weights"):
        fresh.stage_backward(km, pm, mask)
    fresh.load_state_dict(r["sd"])
    with pytest.raises(ValueError, match="retaining forward"):
        fresh.stage_backward(km, pm, mask)
    fresh.train_forward(r["xc"][:1].contiguous())
    with pytest.raises(ValueError, match="retaining forward"):
        fresh.stage_backward(km, pm, mask)                                # another N
    fresh.train_forward(r["xc"])
    with pytest.raises(ValueError, match="batch_size"):
        fresh.stage_backward(km, pm, mask, batch_size=0)
    fresh.set_skeleton(*tc.skeleton("guide5")[1:], tc.skeleton("guide5")[0])
    with pytest.raises(ValueError, match="skeleton"):
        fresh.stage_backward(km, pm, mask)
    half = Engine(0, nref=1, num_channels=64, dtype=_lib.BF16)
    half.load_state_dict(synth.make_state_dict(1, seed=1, num_channels=64))
    with pytest.raises(ValueError, match="fp32"):
        half.train_forward(torch.zeros(1, 3, 64, 64, device="cuda"))
    km64 = torch.zeros(1, 19, 8, 8, device="cuda")
    with pytest.raises(ValueError, match="fp32"):
        half.stage_backward(km64, torch.zeros(1, 38, 8, 8, device="cuda"), torch.ones(1, 8, 8, device="cuda"))


def test_callers_stream_orders_input_and_results():
    r = run("a")
    eng = r["eng"]
    flat = eng.flat_of(r["grads"]).clone()
    side = torch.cuda.Stream()
    x = torch.zeros_like(r["xc"])
    junk = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(40):
            junk = (junk @ junk) * 1e-3
        x.copy_(r["xc"])                               # the real frames exist only once the stream gets here
        outs = eng.train_forward(x)
        g, d = eng.stage_backward(r["km"], r["pm"], r["mask"])
        total = eng.flat_of(g).sum() + d.sum() + outs[0].sum()      # consumer queued on the caller's stream
        pending = not side.query()
    assert pending                                      # the host ran ahead: nothing above blocked on the device
    side.synchronize()
    assert torch.equal(eng.flat_of(g), flat) and torch.equal(d, r["dfeat"]) and torch.equal(outs[0], r["outs"][0])
    assert float(total) == float(flat.sum() + r["dfeat"].sum() + r["outs"][0].sum())


def test_one_call_wrapper_matches_stage_losses():
    c, NH, NP, sd, x = inputs("a")
    net = PoseEstimationWithMobileNet(num_refinement_stages=c["nref"], num_channels=c["C"])
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    K = tc.skeleton(c["skel"])[0]
    kp, n = bc.persons(c)
    labels = tc.frames_to_labels([[kp[f, i] for i in range(n[f])] for f in range(c["N"])], K)
    full = np.repeat(np.repeat(bc.loss_mask(c), 8, 1), 8, 2)
    want = val.stage_losses(net, x, labels, full)
    losses, grads, dfeat = val.stage_gradients(net, x, labels, full)
    assert losses == want
    r = run("a")
    assert torch.equal(net.engine.flat_of(grads), r["eng"].flat_of(r["grads"])) and torch.equal(dfeat, r["dfeat"])
    with pytest.raises(Exception):
        net.train(True)
