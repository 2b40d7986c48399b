"""CPU: the NumPy restatement of the training targets, the mask mean and the L2 loss (tests/train_cases.py) against what the
reference's own statements produced (tests/golden/train_*.npz, tools/make_train_golden.py), the label marshalling of the
datasets.coco drop-in, and the argument checks of the new exports that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.datasets import coco as coco_mod
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet

import train_cases as tc
from conftest import GOLDEN

TARGET_FILES = tc.TARGET_FILES
ALL_CASES = [(f, c) for f, names in TARGET_FILES.items() for c in names]
OLD_CASES = [(f, c) for f, c in ALL_CASES if f != "train_targets_grid"]


@pytest.fixture(scope="module")
def cases():
    return tc.all_cases()


@pytest.fixture(scope="module")
def golden():
    return {f: np.load(os.path.join(GOLDEN, f + ".npz")) for f in list(TARGET_FILES) + ["train_loss", "train_loss_grid"]}


def test_the_old_case_table_is_untouched_by_the_grid_cases(cases):
    old = tc.build_cases()
    assert sorted(old) == sorted(c for _, c in OLD_CASES) and sorted(cases) == sorted(c for _, c in ALL_CASES)
    for name in old:
        assert cases[name][:6] == old[name][:6]
        assert all(np.array_equal(p, q) for f, g in zip(cases[name][6], old[name][6]) for p, q in zip(f, g))


def test_fixture_inputs_are_the_case_table(cases, golden):
    for f, name in ALL_CASES:
        skel, H, W, stride, sigma, thick, frames = cases[name]
        K = tc.skeleton(skel)[0]
        kpts, n = tc.frames_to_arrays(frames, K)
        g = golden[f]
        assert list(g["cases"]) == TARGET_FILES[f]
        assert g[name + ":geometry"].tolist() == [H, W, stride, K] and g[name + ":sigma_thickness"].tolist() == [sigma, thick]
        assert np.array_equal(g[name + ":kpts"], kpts) and np.array_equal(g[name + ":n_persons"], n)


@pytest.mark.parametrize("fname,name", ALL_CASES)
def test_vectorised_restatement_matches_the_reference(cases, golden, fname, name):
    """Touched pixels identical; values within 1 float32 ulp (np.exp against math.exp may differ in the last double bit)."""
    skel, H, W, stride, sigma, thick, frames = cases[name]
    K, lk, lp = tc.skeleton(skel)
    g = golden[fname]
    km, pm = tc.targets(g[name + ":kpts"], g[name + ":n_persons"], H, W, stride, sigma, thick, K, tc.limb_rows(lk, lp))
    for got, want in ((km, g[name + ":keypoint_maps"]), (pm, g[name + ":paf_maps"])):
        assert got.shape == want.shape and got.dtype == np.float32
        assert np.array_equal(tc.touched(got), tc.touched(want))
        u = tc.ulp_distance(got, want)
        print(name, "non-identical elements:", int((u > 0).sum()), "of", u.size)
        assert u.max() <= 1


@pytest.mark.parametrize("fname,name", [("train_targets", "borders"), ("train_targets", "paf_t2"), ("train_targets_custom", "guide5"),
                                        ("train_targets_grid", "interior"), ("train_targets_grid", "chain33")])
def test_pixel_loop_restatement_is_bit_identical(cases, golden, fname, name):
    skel, H, W, stride, sigma, thick, _ = cases[name]
    K, lk, lp = tc.skeleton(skel)
    g = golden[fname]
    km, pm = tc.targets_loops(g[name + ":kpts"], g[name + ":n_persons"], H, W, stride, sigma, thick, K, tc.limb_rows(lk, lp))
    assert np.array_equal(km, g[name + ":keypoint_maps"]) and np.array_equal(pm, g[name + ":paf_maps"])


def test_goldens_hold_what_the_cases_are_for(golden):
    g = golden["train_targets"]
    k, p = g["borders:keypoint_maps"], g["borders:paf_maps"]
    assert g["borders:n_persons"].tolist() == [3, 0, 1]
    assert not k[1, :18].any() and (k[1, 18] == 1).all() and not p[1].any()
    assert k[0, 0, 0, 0] == 1.0 and (k[0, :18] == 1.0).sum() > 3
    assert g["odd_45x43:keypoint_maps"].shape[2:] == (5, 5) and g["stride4_sigma3p5:keypoint_maps"].shape[2:] == (12, 10)
    assert g["chunk:n_persons"].tolist() == [tc.CHUNK - 1, tc.CHUNK, tc.CHUNK + 1]
    a, b = g["cross_ab:paf_maps"], g["cross_ba:paf_maps"]
    assert not np.array_equal(a, b) and np.array_equal(a != 0, b != 0)
    assert np.array_equal(g["cross_ab:kpts"][:, ::-1], g["cross_ba:kpts"])


def test_grid_goldens_hold_what_the_cases_are_for(cases, golden):
    g = golden["train_targets_grid"]
    tc.check_grid_cases(cases, {name: (g[name + ":keypoint_maps"], g[name + ":paf_maps"]) for name in tc.GRID_CASES})
    for name in ("chain33", "chain64"):
        K, lk, lp = tc.skeleton(name)
        assert K == int(name[5:]) and lk == [[j, j + 1] for j in range(K - 1)] and lp == [[2 * j, 2 * j + 1] for j in range(K - 1)]
        assert g[name + ":keypoint_maps"].shape[1] == K + 1 and g[name + ":paf_maps"].shape[1] == 2 * (K - 1)
        assert sorted(set(g[name + ":kpts"][..., 2].ravel().tolist())) == [0.0, 1.0, 2.0]
        assert tc.CHUNK * K > 256                                         # a full chunk needs a second staging trip ...
    assert tc.CHUNK * 32 <= 256                                           # ... and 33 is the smallest such K


# ---- mutants of tc.targets: each is the restatement with one of the kernel's forms left out.  It must pass the fixture check on
# every old case (the suite without the grid cases cannot tell it from the real thing) and fail it on the named new ones.
def _agrees(got, want):
    return all(np.array_equal(tc.touched(a), tc.touched(b)) and tc.ulp_distance(a, b).max() <= 1 for a, b in zip(got, want))


def _restated(cases, g, name, kpts=None):
    skel, H, W, stride, sigma, thick, _ = cases[name]
    K, lk, lp = tc.skeleton(skel)
    kpts = g[name + ":kpts"] if kpts is None else kpts
    return tc.targets(kpts, g[name + ":n_persons"], H, W, stride, sigma, thick, K, tc.limb_rows(lk, lp))


def mutant_one_workgroup(km, pm):
    """Pixels of linear index 256 or above stay as an empty frame gives them: key-point channels 0, background 1, PAF 0."""
    km, pm = km.copy(), pm.copy()
    N, C, h, w = km.shape
    fk, fp = km.reshape(N, C, h * w), pm.reshape(N, -1, h * w)
    fk[:, :-1, 256:] = 0
    fk[:, -1, 256:] = 1
    fp[:, :, 256:] = 0
    return km, pm


def mutant_wrapped_index(km, pm):
    """Pixel i at 256 or above takes pixel i - 256's value."""
    out = []
    for m in (km, pm):
        N, C, h, w = m.shape
        f = m.reshape(N, C, h * w).copy()
        f[:, :, 256:] = m.reshape(N, C, h * w)[:, :, :max(h * w - 256, 0)]
        out.append(f.reshape(m.shape))
    return tuple(out)


def mutant_one_staging_trip(kpts, K):
    """Inside each chunk of CHUNK persons, entries q * K + k >= 256 were never staged: they count as visibility 2."""
    kpts = kpts.copy()
    q = np.arange(kpts.shape[1])[:, None] % tc.CHUNK
    late = q * K + np.arange(K)[None, :] >= 256
    kpts[:, late, 2] = 2.0
    return kpts


# not full256: 256 pixels exactly is what that case is for; the chains' scattered key-points reach their 17th map row as well
PIXEL_MUTANT_DIFFERS = set(tc.PAST_256) | {"chain33", "chain64"}
STAGING_MUTANT_DIFFERS = {"chain33", "chain64"}


@pytest.mark.parametrize("fname,name", ALL_CASES)
def test_mutants_pass_every_old_case_and_fail_the_named_new_ones(cases, golden, fname, name):
    g = golden[fname]
    want = (g[name + ":keypoint_maps"], g[name + ":paf_maps"])
    km, pm = _restated(cases, g, name)
    assert _agrees((km, pm), want)
    K = tc.skeleton(cases[name][0])[0]
    got = {"one workgroup": _agrees(mutant_one_workgroup(km, pm), want),
           "wrapped index": _agrees(mutant_wrapped_index(km, pm), want),
           "one staging trip": _agrees(_restated(cases, g, name, mutant_one_staging_trip(g[name + ":kpts"], K)), want)}
    expect = {"one workgroup": name not in PIXEL_MUTANT_DIFFERS, "wrapped index": name not in PIXEL_MUTANT_DIFFERS,
              "one staging trip": name not in STAGING_MUTANT_DIFFERS}
    assert got == expect, name
    if fname != "train_targets_grid":
        assert all(got.values())


def test_default_skeleton_gives_the_reference_channel_layout():
    K, lk, lp = tc.skeleton("coco")
    assert tc.train_limbs(lk, lp) == coco_mod.BODY_PARTS_KPT_IDS == tc.COCO_TRAIN_LIMBS
    assert lp[lk.index([1, 2])] == [12, 13]


def test_mask_mean_is_exact_for_binary_masks():
    rng = np.random.RandomState(3)
    m = (rng.rand(2, 48, 40) > 0.4).astype(np.float32)
    m[1, 8:16, 8:16] = 0
    for s in (8, 4):
        got = tc.mask_mean(m, s)
        want = m.reshape(2, 48 // s, s, 40 // s, s).astype(np.int64).sum(axis=(2, 4)) / float(s * s)      # integer block sums
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert tc.mask_mean(m, 8)[1, 1, 1] == 0


@pytest.mark.parametrize("case", tc.MASK_CASES)
def test_mask_mean_sums_exactly_on_the_gpu_cases(case):
    """The masks of tests/test_gpu_train.py: 0 / 1, and multiples of 2^-8 in [0, 1].  256 times a block's sum is an integer below
    2^17, so the float64 sum of mask_mean is exact in any order and the mean is that sum divided once."""
    N, H, W, s = case
    for kind in ("binary", "fraction"):
        m = tc.mask_input(case, kind)
        scaled = m.astype(np.float64) * 256
        assert m.dtype == np.float32 and m.min() >= 0 and m.max() <= 1 and np.array_equal(scaled, np.round(scaled))
        assert (kind == "binary") == (set(np.unique(m).tolist()) <= {0.0, 1.0}) and len(np.unique(m)) > 1
        isum = scaled.astype(np.int64).reshape(N, H // s, s, W // s, s).sum(axis=(2, 4))                  # integer block sums
        assert isum.max() <= 256 * s * s <= 1 << 16
        want = ((isum.astype(np.float64) / 256.0) / float(s * s)).astype(np.float32)
        got = tc.mask_mean(m, s)
        assert got.shape == (N, H // s, W // s) and np.array_equal(got, want)


def test_a_loss_that_stops_at_the_grid_cap_passes_the_old_cases_only(golden):
    """The mutant sums the first 262 144 positions (one trip of the capped grid).  n * 2^-52 relative is the GPU tests' bar."""
    def miss(name, n_stages):
        outs, kt, pt, mask = tc.loss_inputs(name, n_stages)
        worst = 0.0
        for i, o in enumerate(outs):
            t = pt if i % 2 else kt
            want = tc.l2_loss64(o, t, mask, kt.shape[0])
            worst = max(worst, abs(tc.l2_loss64_first(o, t, mask, kt.shape[0], tc.LOSS_CAP) - want) / (o.size * 2.0 ** -52 * want))
        return worst
    for name in tc.LOSS_CASES:
        assert miss(name, int(golden["train_loss"][name + ":n_stages"])) == 0.0
    assert miss("cap_exact", 1) == 0.0 and miss("s18", 9) == 0.0
    assert miss("one_past_cap", 1) > 1 and miss("second_trip", 1) > 1
    N, CH, CP, h, w, _ = tc.LOSS_GRID_CASES["cap_exact"]
    assert N * h * w == tc.LOSS_CAP
    assert [c[0] * c[3] * c[4] for c in (tc.LOSS_GRID_CASES["one_past_cap"], tc.LOSS_GRID_CASES["second_trip"])] == [tc.LOSS_CAP + 1, 263538]
    # one_past_cap: the last position alone carries more than the bar
    outs, kt, pt, mask = tc.loss_inputs("one_past_cap", 1)
    assert mask[-1, -1, -1] == 1 and np.array_equal(outs[0][-1, :, -1, -1], kt[-1, :, -1, -1] + np.float32(1))
    assert np.abs(outs[0] - kt).reshape(-1, kt.shape[1], 52429)[..., :-1].max() < 0.75


def test_float64_loss_matches_the_reference_float32_loss(golden):
    """(n + 8) * 2^-24 relative: any float32 summation order over n non-negative terms, plus the roundings of one term."""
    g = golden["train_loss"]
    for name in tc.LOSS_CASES:
        outs, kt, pt, mask = tc.loss_inputs(name, int(g[name + ":n_stages"]))
        assert np.array_equal(g[name + ":digest"], [float(a.astype(np.float64).sum()) for a in outs + [kt, pt, mask]])
        for i, o in enumerate(outs):
            want = float(g[name + ":losses_f32"][i])
            got = tc.l2_loss64(o, pt if i % 2 else kt, mask, kt.shape[0])
            print(name, i, got, want)
            assert abs(got - want) <= (o.size + 8) * 2.0 ** -24 * got
    g = golden["train_loss_grid"]                         # 18 tensors on the 6 x 5 maps
    assert list(g["cases"]) == ["s18"] and int(g["s18:n_stages"]) == tc.LOSS_GRID_STAGES["s18"] == 9
    outs, kt, pt, mask = tc.loss_inputs("s18", 9)
    assert len(outs) == 18 and np.array_equal(g["s18:digest"], [float(a.astype(np.float64).sum()) for a in outs + [kt, pt, mask]])
    for i, o in enumerate(outs):
        want = float(g["s18:losses_f32"][i])
        got = tc.l2_loss64(o, pt if i % 2 else kt, mask, kt.shape[0])
        assert abs(got - want) <= (o.size + 8) * 2.0 ** -24 * got


def test_labels_to_arrays_keeps_label_order(cases):
    frames = cases["borders"][6]
    kpts, n = coco_mod.labels_to_arrays(tc.frames_to_labels(frames, 18), 18)
    want, wn = tc.frames_to_arrays(frames, 18)
    assert n.tolist() == [3, 1, 1] and kpts.dtype == np.float64             # the format has no frame without a main person
    assert np.array_equal(kpts[0], want[0]) and np.array_equal(kpts[2, :1], want[2, :1]) and (kpts[1, 0, :, 2] == 2).all()
    with pytest.raises(ValueError):
        coco_mod.labels_to_arrays([{"keypoints": [[0, 0, 1]] * 17}], 18)


def test_argument_checks_that_need_no_gpu():
    L = _lib.lib()
    buf = (C.c_float * 16)()
    one = (C.c_int * 1)(0)
    assert L.lwp_mask_downsample(None, buf, 0, 1, 45, 40, 8, buf) == _lib.LWP_ERR_ARG
    assert b"whole number" in L.lwp_last_error(None)
    assert L.lwp_mask_downsample(None, buf, 0, 1, 48, 43, 8, buf) == _lib.LWP_ERR_ARG
    assert L.lwp_mask_downsample(None, buf, 0, 1, 48, 40, 8, buf) == _lib.LWP_ERR_ARG and b"handle" in L.lwp_last_error(None)
    assert L.lwp_train_targets(None, None, 0, one, 1, 0, 48, 40, 8, 0.0, 1.0, buf, buf) == _lib.LWP_ERR_ARG
    assert b"sigma" in L.lwp_last_error(None)
    one[0] = 2
    assert L.lwp_train_targets(None, None, 0, one, 1, 1, 48, 40, 8, 7.0, 1.0, buf, buf) == _lib.LWP_ERR_ARG
    assert b"persons" in L.lwp_last_error(None)
    assert L.lwp_stage_losses(None, None, 4, buf, buf, buf, 1, 6, 5, 1, None) == _lib.LWP_ERR_ARG
    # more than 2^28 map cells (the kernels index a map with int): 2^14 x 2^15 cells at stride 1
    one[0] = 0
    assert L.lwp_train_targets(None, None, 0, one, 1, 0, 1 << 14, 1 << 15, 1, 7.0, 1.0, buf, buf) == _lib.LWP_ERR_ARG
    assert b"2^28" in L.lwp_last_error(None)
    assert L.lwp_mask_downsample(None, buf, 1, 1, 1 << 14, 1 << 15, 1, buf) == _lib.LWP_ERR_ARG and b"2^28" in L.lwp_last_error(None)
    ms = C.c_float()
    assert L.lwp_time_train_targets(None, None, 0, one, 1, 0, 48, 40, 8, 7.0, 1.0, buf, buf, 0, C.byref(ms)) == _lib.LWP_ERR_ARG
    assert L.lwp_time_stage_losses(None, None, 4, buf, buf, buf, 1, 6, 5, 1, 3, None) == _lib.LWP_ERR_ARG


def test_training_mode_still_raises():
    with pytest.raises(NotImplementedError):
        PoseEstimationWithMobileNet().train(True)
