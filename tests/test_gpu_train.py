"""Training targets, mask and per-stage loss on the GPU (-m gpu), every call through the C-ABI.

Targets against what the reference's own statements produced (tests/golden/train_targets*.npz): the set of touched pixels
identical, every value within 1 float32 ulp (the device's exp / sqrt stand in for CPython's exp / pow; a double that is off
in its last bit moves a float32 rounding by one step at most); the count of non-identical elements is printed.  Mask: exact.
Loss: relative error <= n * 2^-52 against the float64 restatement on the same float32 inputs (n non-negative terms summed in
double), <= (n + 8) * 2^-24 against the reference's float32 l2_loss, and the same bits from two calls.

train_targets_grid.npz, the mask cases of train_cases.MASK_CASES and the loss cases of train_cases.LOSS_GRID_CASES take the
kernels past their smallest form at the same bars: more than one workgroup per frame, a second trip of the targets kernel's
staging loop (K = 33, 64), a second trip of the loss grid (more than 262 144 positions) and a second loss launch (18 tensors).
tests/test_train_host.py shows that a restatement without one of these forms fails on those cases."""
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth, val
from lwpose_amd.datasets import coco as coco_mod
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.modules.loss import l2_loss
from lwpose_amd.runtime import Engine

import train_cases as tc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = tc.all_cases()
_engines = {}


def engine(skel="coco", nref=1):
    """One engine per (skeleton, stage count); custom key-point sets (the chains too: 34 + 64 and 65 + 126 channels) get
    num_heatmaps = K + 1, num_pafs = 2L and their table."""
    if (skel, nref) not in _engines:
        K, lk, lp = tc.skeleton(skel)
        if skel == "coco":
            e = Engine(0, nref=nref)
        else:
            e = Engine(0, nref=nref, num_heatmaps=K + 1, num_pafs=2 * len(lk))
            e.set_skeleton(lk, lp, K)
        _engines[(skel, nref)] = e
    return _engines[(skel, nref)]


@pytest.fixture(scope="module")
def golden():
    return {f: np.load(os.path.join(GOLDEN, f + ".npz")) for f in list(tc.TARGET_FILES) + ["train_loss", "train_loss_grid"]}


def check_targets(name, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(tc.touched(got), tc.touched(want)), name
    u = tc.ulp_distance(got, want)
    print("%s: %d of %d elements not bit-identical" % (name, int((u > 0).sum()), u.size))
    assert u.max() <= 1, name


# ------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("fname,name", [(f, c) for f, names in tc.TARGET_FILES.items() for c in names])
def test_targets_match_the_reference(golden, fname, name):
    skel, H, W, stride, sigma, thick, _ = CASES[name]
    g = golden[fname]
    eng = engine(skel)
    kpts, n = g[name + ":kpts"], g[name + ":n_persons"]
    km, pm = eng.train_targets(kpts, n, (H, W), stride, sigma, thick)                 # host key-points
    check_targets(name + " keypoint_maps", km, g[name + ":keypoint_maps"])
    check_targets(name + " paf_maps", pm, g[name + ":paf_maps"])
    km2, pm2 = eng.train_targets(torch.from_numpy(kpts).cuda(0), n, (H, W), stride, sigma, thick)   # device key-points
    assert torch.equal(km, km2) and torch.equal(pm, pm2)


def test_crossing_limbs_follow_the_label_order(golden):
    g = golden["train_targets"]
    eng = engine()
    out = {}
    for name in ("cross_ab", "cross_ba"):
        _, H, W, stride, sigma, thick, _ = CASES[name]
        out[name] = eng.train_targets(g[name + ":kpts"], g[name + ":n_persons"], (H, W), stride, sigma, thick)[1].cpu().numpy()
        check_targets(name, torch.from_numpy(out[name]), g[name + ":paf_maps"])
    assert not np.array_equal(out["cross_ab"], out["cross_ba"])


def test_rows_beyond_a_frames_count_and_no_person_at_all(golden):
    g = golden["train_targets"]
    kpts, n = g["borders:kpts"].copy(), g["borders:n_persons"]
    kpts[1] = kpts[0]                                   # frame 1 counts 0 persons: its rows must not be read
    kpts[2, 1:] = kpts[0, 1:]
    km, pm = engine().train_targets(kpts, n, (48, 40))
    check_targets("ragged keypoint_maps", km, g["borders:keypoint_maps"])
    check_targets("ragged paf_maps", pm, g["borders:paf_maps"])
    km, pm = engine().train_targets(np.zeros((2, 0, 18, 3)), [0, 0], (48, 40))         # Pmax = 0
    assert not km[:, :18].any() and bool((km[:, 18] == 1).all()) and not pm.any()


def test_generate_targets_drop_in_and_broadcast_masks(golden):
    g = golden["train_targets"]
    frames = CASES["chunk"][6]
    mask = (np.random.RandomState(4).rand(3, 48, 40) > 0.3).astype(np.float32)
    t = coco_mod.generate_targets(engine(), tc.frames_to_labels(frames, 18), (48, 40), mask)
    check_targets("drop-in keypoint_maps", t["keypoint_maps"], g["chunk:keypoint_maps"])
    check_targets("drop-in paf_maps", t["paf_maps"], g["chunk:paf_maps"])
    assert tuple(t["keypoint_mask"].shape) == (3, 19, 6, 5) and tuple(t["paf_mask"].shape) == (3, 38, 6, 5)
    assert t["keypoint_mask"].stride(1) == 0 and t["paf_mask"].stride(1) == 0          # views, not copies
    assert np.array_equal(t["paf_mask"][:, 7].cpu().numpy(), tc.mask_mean(mask, 8))
    ones = coco_mod.generate_targets(engine(), tc.frames_to_labels(frames, 18), (48, 40))
    assert bool((ones["keypoint_mask"] == 1).all())


def test_targets_argument_checks():
    eng = engine()
    with pytest.raises(ValueError):
        eng.train_targets(np.zeros((1, 1, 17, 3)), [1], (48, 40))
    with pytest.raises(ValueError):
        eng.train_targets(np.zeros((1, 1, 18, 3)), [2], (48, 40))
    with pytest.raises(ValueError):
        eng.train_targets(np.zeros((1, 1, 18, 3)), [1], (48, 40), sigma=0)
    bad = np.zeros((1, 1, 18, 3))
    bad[0, 0, 3, 0] = np.nan
    with pytest.raises(ValueError):
        eng.train_targets(bad, [1], (48, 40))


def test_targets_refuse_a_paf_channel_of_two_limbs():
    """The kernel walks the limbs inside a chunk of persons, the reference limb by limb; the orders agree only while every
    target channel belongs to one limb, so any other table is refused."""
    K, lk, lp = tc.skeleton("coco")
    lp = [list(r) for r in lp]
    lp[3] = list(lp[2])
    e = Engine(0)
    e.set_skeleton(lk, lp, K)
    with pytest.raises(ValueError, match="another limb"):
        e.train_targets(np.zeros((1, 1, 18, 3)), [1], (48, 40))


# ------------------------------------------------------------------------------------------ mask
@pytest.mark.parametrize("stride", [8, 4])
def test_mask_downsample_is_exact(stride):
    rng = np.random.RandomState(stride)
    mask = (rng.rand(3, 48, 40) > 0.4).astype(np.float32)
    mask[1, 8:24, 8:16] = 0
    want = tc.mask_mean(mask, stride)
    eng = engine()
    assert np.array_equal(eng.mask_downsample(mask, stride).cpu().numpy(), want)
    assert np.array_equal(eng.mask_downsample(torch.from_numpy(mask).cuda(0), stride).cpu().numpy(), want)
    assert np.array_equal(eng.mask_downsample(mask[0], stride).cpu().numpy(), want[0])


@pytest.mark.parametrize("kind", ["binary", "fraction"])
@pytest.mark.parametrize("case", tc.MASK_CASES)
def test_mask_downsample_is_exact_past_one_workgroup(case, kind):
    """More than 256 cells per frame, frame offsets, a 1 x 257 map, an odd stride, stride 1 and 256-cell blocks, bit for bit
    against the float64 block mean rounded once.  The ``fraction`` masks (multiples of 2^-8) go beyond what the reference ever
    feeds, its masks being binary: they pin the kernel's own statement, the double sum of a block divided once, on inputs whose
    sum is exact in any order (tests/test_train_host.py), so that the one correct rounding is the only answer."""
    N, H, W, stride = case
    mask = tc.mask_input(case, kind)
    want = tc.mask_mean(mask, stride)
    eng = engine()
    got = eng.mask_downsample(mask, stride)
    assert tuple(got.shape) == (N, H // stride, W // stride) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(eng.mask_downsample(torch.from_numpy(mask).cuda(0), stride).cpu().numpy(), want)


def test_mask_downsample_refuses_partial_blocks():
    for shape in ((1, 45, 40), (1, 48, 43)):
        with pytest.raises(ValueError, match="whole number"):
            engine().mask_downsample(np.ones(shape, np.float32), 8)


# ------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("name,skel,nref", [("small", "coco", 3), ("multi_block", "coco", 1), ("guide5", "guide5", 1)])
def test_stage_losses_bounds_and_determinism(golden, name, skel, nref):
    g = golden["train_loss"]
    outs, kt, pt, mask = tc.loss_inputs(name, int(g[name + ":n_stages"]))
    assert len(outs) == 2 * (nref + 1) and (mask == 0).any()
    eng = engine(skel, nref)
    d = [torch.from_numpy(o).cuda(0) for o in outs]
    dk, dp, dm = torch.from_numpy(kt).cuda(0), torch.from_numpy(pt).cuda(0), torch.from_numpy(mask).cuda(0)
    N = kt.shape[0]
    got = eng.stage_losses(d, dk, dp, dm, N)
    assert got == eng.stage_losses(d, dk, dp, dm, N)                                   # the same bits twice
    for i, o in enumerate(outs):
        want64 = tc.l2_loss64(o, pt if i % 2 else kt, mask, N)
        want32 = float(g[name + ":losses_f32"][i])
        print(name, i, got[i], want64, want32)
        assert got[i] > 0 and abs(got[i] - want64) <= o.size * 2.0 ** -52 * want64
        assert abs(got[i] - want32) <= (o.size + 8) * 2.0 ** -24 * got[i]
    # strided views are read through a contiguous copy; a None entry is skipped
    wide = torch.zeros(d[0].shape[:3] + (d[0].shape[3] + 3,), device="cuda:0")
    wide[..., 1:-2] = d[0]
    part = eng.stage_losses([wide[..., 1:-2]] + [None] * (len(d) - 1), dk, None, dm, N)
    assert part[0] == got[0] and part[1:] == [0.0] * (len(d) - 1)


def _loss_case_on_device(name, n_stages):
    outs, kt, pt, mask = tc.loss_inputs(name, n_stages)
    d = [torch.from_numpy(o).cuda(0) for o in outs]
    want = [tc.l2_loss64(o, pt if i % 2 else kt, mask, kt.shape[0]) for i, o in enumerate(outs)]
    return outs, d, torch.from_numpy(kt).cuda(0), torch.from_numpy(pt).cuda(0), torch.from_numpy(mask).cuda(0), kt.shape[0], want


def _check_losses(name, got, want, outs):
    """|got - want64| <= n * 2^-52 * want64 per tensor; prints the worst error in units of that bar."""
    worst = 0.0
    for i, o in enumerate(outs):
        bar = o.size * 2.0 ** -52 * want[i]
        worst = max(worst, abs(got[i] - want[i]) / bar)
        assert got[i] > 0 and abs(got[i] - want[i]) <= bar, (name, i, got[i], want[i])
    print("%s: worst loss error %.3g of its bar" % (name, worst))


@pytest.mark.parametrize("name", ["cap_exact", "one_past_cap", "second_trip"])
def test_stage_losses_at_and_past_the_grid_cap(name):
    """262 144 positions fill the capped grid's one trip exactly; 262 145 leave one position to the second trip, which carries an
    error of 1 where every other error is of order 0.1 (its term alone is many times the bar); 2 x 363 x 363 is a second trip
    of 1394 positions across a frame boundary."""
    N, CH, CP, h, w, _ = tc.LOSS_GRID_CASES[name]
    assert (N * h * w > tc.LOSS_CAP) == (name != "cap_exact")
    outs, d, dk, dp, dm, N, want = _loss_case_on_device(name, 1)
    eng = engine("guide5", 0)
    got = eng.stage_losses(d, dk, dp, dm, N)
    assert got == eng.stage_losses(d, dk, dp, dm, N)                                   # the same bits twice
    _check_losses(name, got, want, outs)


@pytest.mark.parametrize("name", ["s18", "s18_46"])
def test_stage_losses_of_18_tensors_take_two_launches(golden, name):
    """8 refinement stages: tensors 16 and 17 come from the second launch, which writes behind the first launch's sums and
    reuses its partials (46 x 46: of more than one workgroup)."""
    outs, d, dk, dp, dm, N, want = _loss_case_on_device(name, tc.LOSS_GRID_STAGES[name])
    assert len(outs) == 18
    eng = engine("guide5", 8)
    got = eng.stage_losses(d, dk, dp, dm, N)
    assert got == eng.stage_losses(d, dk, dp, dm, N)
    _check_losses(name, got, want, outs)
    assert len(set(got)) == 18                                                         # no sum landed in two places
    if name == "s18":
        g = golden["train_loss_grid"]
        for i, o in enumerate(outs):
            assert abs(got[i] - float(g["s18:losses_f32"][i])) <= (o.size + 8) * 2.0 ** -24 * got[i]
    part = eng.stage_losses(d[:16] + [None, d[17]], dk, dp, dm, N)                     # a None entry in the second launch
    assert part[:16] == got[:16] and part[16] == 0.0 and part[17] == got[17]
    part = eng.stage_losses([None] * 16 + d[16:], dk, dp, dm, N)                       # nothing for the first launch to do
    assert part[:16] == [0.0] * 16 and part[16:] == got[16:]


def test_l2_loss_drop_in(golden):
    outs, kt, pt, mask = tc.loss_inputs("small", 2)
    dm = torch.from_numpy(mask).cuda(0)
    full = dm[:, None].expand(-1, 38, -1, -1).contiguous()                              # a mask copied into every channel, as the reference does
    v = l2_loss(torch.from_numpy(outs[1]).cuda(0), torch.from_numpy(pt).cuda(0), full, 2)
    assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 0
    want = tc.l2_loss64(outs[1], pt, mask, 2)
    assert abs(v.item() - want) <= outs[1].size * 2.0 ** -52 * want
    v = l2_loss(torch.from_numpy(outs[0]).cuda(0), torch.from_numpy(kt).cuda(0), dm[:, None].expand(-1, 19, -1, -1), 2)
    want = tc.l2_loss64(outs[0], kt, mask, 2)
    assert abs(v.item() - want) <= outs[0].size * 2.0 ** -52 * want
    full[0, 3, 0, 0] += 1
    with pytest.raises(ValueError, match="differs between channels"):
        l2_loss(torch.from_numpy(outs[1]).cuda(0), torch.from_numpy(pt).cuda(0), full, 2)


def test_stage_losses_argument_checks():
    outs, kt, pt, mask = tc.loss_inputs("small", 2)
    d = [torch.from_numpy(o).cuda(0) for o in outs]
    dk, dp, dm = torch.from_numpy(kt).cuda(0), torch.from_numpy(pt).cuda(0), torch.from_numpy(mask).cuda(0)
    with pytest.raises(ValueError, match="n_outs"):
        engine("coco", 1).stage_losses(d[:2], dk, dp, dm)                               # nref 1 returns 4 tensors
    with pytest.raises(ValueError, match="n_outs"):
        engine("coco", 3).stage_losses(d, dk, dp, dm)
    e = Engine(0)                                                                       # 19 / 38 channels, but a 5-type skeleton
    K, lk, lp = tc.skeleton("guide5")
    e.set_skeleton(lk, lp, K)
    with pytest.raises(ValueError, match="skeleton"):
        e.stage_losses(d, dk, dp, dm)
    with pytest.raises(ValueError):
        engine("coco", 1).stage_losses(d, dk, dp, dm[:, :3])                            # mask of another size


# ------------------------------------------------------------------------------------------ end to end
def _net_input(n, h, w, seed):
    fr = synth.make_frames(n, h, w, seed0=seed)
    return np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))


@pytest.mark.parametrize("nref,dtype", [(1, "fp32"), (3, "fp32"), (1, "fp16")])
def test_val_stage_losses_end_to_end(nref, dtype):
    """forward + targets + loss in one call at the net_small fixture size (2 x 64 x 96), against float64 NumPy over the HIP
    net's own copied-back outputs and the oracle's targets."""
    net = PoseEstimationWithMobileNet(num_refinement_stages=nref, dtype=dtype)
    load_state(net, {"state_dict": synth.make_state_dict(nref, seed=1)})
    net.eval().cuda(0)
    x = _net_input(2, 64, 96, seed=100)
    rng = np.random.RandomState(9)
    frames = tc._crowd(rng, "coco", 64, 96, [3, tc.CHUNK + 2])
    mask = (rng.rand(2, 64, 96) > 0.2).astype(np.float32)
    got = val.stage_losses(net, x, tc.frames_to_labels(frames, 18), mask)
    assert len(got) == 2 * (nref + 1)
    outs = [o.cpu().numpy() for o in net(torch.from_numpy(x).cuda(0))]
    K, lk, lp = tc.skeleton("coco")
    kpts, n = tc.frames_to_arrays(frames, K)
    kt, pt = tc.targets(kpts, n, 64, 96, 8, 7, 1, K, tc.limb_rows(lk, lp))
    small = tc.mask_mean(mask, 8)
    for i, o in enumerate(outs):
        want = tc.l2_loss64(o, pt if i % 2 else kt, small, 2)
        print(dtype, nref, i, got[i], want)
        # the oracle's targets may differ from the device's by 1 float32 ulp per element (exp): every target lies in [-1, 1],
        # where a float32 step is at most e = 2^-24, so with d = out - t a term (d m)^2 / 2 / batch moves by at most
        # (2 |d| e + e^2) m^2 / 2 / batch; the float64 summation adds n * 2^-52 relative
        d = np.abs(o.astype(np.float64) - (pt if i % 2 else kt))
        e = 2.0 ** -24
        slack = float(((2 * d * e + e * e) * small[:, None].astype(np.float64) ** 2).sum()) / 2 / 2
        assert abs(got[i] - want) <= o.size * 2.0 ** -52 * want + slack
    assert got == val.stage_losses(net, x, tc.frames_to_labels(frames, 18), mask)
