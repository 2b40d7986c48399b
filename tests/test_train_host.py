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

TARGET_FILES = {"train_targets": tc.COCO_CASES, "train_targets_custom": tc.CUSTOM_CASES}
ALL_CASES = [(f, c) for f, names in TARGET_FILES.items() for c in names]


@pytest.fixture(scope="module")
def cases():
    return tc.build_cases()


@pytest.fixture(scope="module")
def golden():
    return {f: np.load(os.path.join(GOLDEN, f + ".npz")) for f in list(TARGET_FILES) + ["train_loss"]}


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


@pytest.mark.parametrize("fname,name", [("train_targets", "borders"), ("train_targets", "paf_t2"), ("train_targets_custom", "guide5")])
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
