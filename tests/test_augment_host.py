"""CPU: the host half of the training augmentation (lwpose_amd.datasets.transformations).  The five classes and plan_batch
against what the reference's own Python produced (tests/golden/augment_cases.npz, tools/make_augment_golden.py): labels,
sizes, crop geometry, the order of the random draws and the dtype conversions are pinned bit for bit.  The pixel routines
restate OpenCV and cannot be pinned here; they get hand-derived checks that do not depend on the restatement being
self-consistent.  And the argument checks of the two new exports that need no GPU, and what the batches of
augment_branch_cases.py are: the conditions under which each reaches the kernel path it is named for."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.datasets import transformations as T

import augment_branch_cases as bc
import augment_cases as ac

CASES = list(range(ac.n_cases()))
PAD = (128, 128, 128)


# ------------------------------------------------------------------------------------------ 1. the reference pin
def check_labels(label, exp):
    kpts, objpos, img_wh = ac.label_arrays(label)
    assert kpts.shape == exp["kpts"].shape and np.array_equal(kpts, exp["kpts"])
    assert np.array_equal(objpos, exp["objpos"])
    assert np.array_equal(img_wh, exp["img_wh"])


@pytest.mark.parametrize("i", CASES)
def test_classes_reproduce_the_reference_bit_for_bit(i):
    sample, transforms, seed, exp = ac.case(i)
    random.seed(seed)
    for t in transforms:
        sample = t(sample)
    state = random.getstate()
    assert sample["image"].dtype == np.uint8 and np.array_equal(sample["image"], exp["image"])
    assert sample["mask"].dtype == np.uint8 and np.array_equal(sample["mask"], exp["mask"])
    small = T.mask_small_u8(sample["mask"], 8)
    assert small.dtype == np.float32 and np.array_equal(small, exp["mask_small"])
    check_labels(sample["label"], exp)
    assert np.array_equal(np.array(state[1], dtype=np.uint64), exp["state"]) and state[2] is None


@pytest.mark.parametrize("i", CASES)
def test_plan_batch_reproduces_the_reference_bit_for_bit(i):
    sample, transforms, seed, exp = ac.case(i)
    before = copy.deepcopy(sample["label"])
    random.seed(seed)
    plan = T.plan_batch([sample], transforms)
    state = random.getstate()
    assert sample["label"] == before                                     # the caller's label is not touched
    image, mask, small = T.apply_plan_host(plan, 8)
    assert image.dtype == np.float32 and np.array_equal(image[0], ac.network_image(exp["image"]))
    assert mask.dtype == np.uint8 and np.array_equal(mask[0], exp["mask"])
    assert small.dtype == np.float32 and np.array_equal(small[0], exp["mask_small"])
    check_labels(plan.labels[0], exp)
    assert plan.kpts.dtype == np.float64 and np.array_equal(plan.kpts[0, :plan.n_persons[0]], exp["kpts"])
    assert plan.n_persons.tolist() == [len(exp["kpts"])]
    assert np.array_equal(np.array(state[1], dtype=np.uint64), exp["state"])


def test_plan_batch_draws_sample_by_sample_from_a_given_rng():
    """Two cases of one crop size in one batch: the draws of the first sample come before those of the second, and an object
    with .random() replaces the global generator (which then stays untouched)."""
    (s0, tr, seed0, e0), (s2, _, _, _) = ac.case(0), ac.case(2)
    random.seed(5)
    untouched = random.getstate()
    rng = random.Random(seed0)
    plan = T.plan_batch([s0, s2], tr, rng)
    assert random.getstate() == untouched
    image, mask, _ = T.apply_plan_host(plan, 8)
    assert np.array_equal(mask[0], e0["mask"]) and np.array_equal(image[0], ac.network_image(e0["image"]))
    follow = random.Random(seed0)
    T.plan_batch([ac.case(0)[0]], tr, follow)
    alone = T.plan_batch([ac.case(2)[0]], tr, follow)                    # the second sample alone, from where the first left the rng
    assert np.array_equal(plan.kpts[1, :plan.n_persons[1]], alone.kpts[0, :alone.n_persons[0]])
    assert rng.getstate() == follow.getstate()


def test_the_fixture_set_keeps_its_coverage():
    others, flips, origin, outside, none_masks, pads = set(), set(), 0, 0, 0, []
    assert len(CASES) >= 12
    for i in CASES:
        sample, transforms, seed, exp = ac.case(i)
        random.seed(seed)
        plan = T.plan_batch([sample], transforms)
        others.add(int(plan.n_persons[0]) - 1)
        flips.add(bool(plan.records[0]["flip"]))
        raw = np.array(sample["label"]["keypoints"], dtype=np.float64)
        h, w = sample["image"].shape[:2]
        origin += int(np.any((raw[:, 0] == 0) & (raw[:, 1] == 0)))
        outside += int(np.any((raw[:, 0] < 0) | (raw[:, 0] >= w) | (raw[:, 1] < 0) | (raw[:, 1] >= h)))
        none_masks += sample["mask"] is None
        pads.append(float(np.all(exp["image"] == np.array(PAD, np.uint8), axis=2).mean()))
        assert tuple(exp["image"].shape[:2]) in ((16, 24), (24, 16))
    assert others == {0, 1, 2} and flips == {False, True} and origin and outside and none_masks
    assert min(pads) < 0.05 and max(pads) > 0.4


# ------------------------------------------------------------------------------------------ 2. crop quirks
crop_sample = ac.crop_sample                                             # shared with the branch cases (augment_branch_cases.py)


def crop_both_ways(sample, crop=16):
    """CropPad alone with center_perterb_max = 0, through the class and through plan_batch; both results."""
    t = T.CropPad(pad=PAD, center_perterb_max=0, crop_x=crop, crop_y=crop)
    plan = T.plan_batch([sample], [t], random.Random(0))
    image, mask, _ = T.apply_plan_host(plan, 8)
    one = t(copy.deepcopy(sample))
    assert np.array_equal(ac.network_image(one["image"]), image[0]) and np.array_equal(one["mask"], mask[0])
    assert one["label"] == plan.labels[0]
    return one, plan.records[0]


def test_tall_image_with_row_start_past_the_width_is_all_pad():
    sample = crop_sample(60, 20, (10.0, 38.0), mask_value=0.0)           # y_start = 30: >= w = 20, < h = 60
    one, g = crop_both_ways(sample)
    assert not g["should_crop"]
    assert np.all(one["image"] == np.array(PAD, np.uint8)) and np.all(one["mask"] == 1)


def test_wide_image_with_row_start_past_the_height_raises_as_the_reference_does():
    sample = crop_sample(20, 60, (30.0, 38.0))                           # y_start = 30: h = 20 < 30 < w = 60
    t = T.CropPad(pad=PAD, center_perterb_max=0, crop_x=16, crop_y=16)
    with pytest.raises(ValueError, match="broadcast"):
        t(copy.deepcopy(sample))
    with pytest.raises(ValueError, match="broadcast"):
        T.plan_batch([sample], [t], random.Random(0))


def test_row_start_at_the_height_and_column_finish_at_zero_copy_nothing():
    for sample in (crop_sample(20, 60, (30.0, 28.0)),                    # y_start = 20 == h
                   crop_sample(20, 60, (-8.0, 10.0))):                   # x_start = -16, x_finish = 0
        one, g = crop_both_ways(sample)
        assert g["should_crop"]
        dy0, dy1, dx0, dx1 = g["dst"]
        assert dy0 == dy1 or dx0 == dx1
        assert np.all(one["image"] == np.array(PAD, np.uint8)) and np.all(one["mask"] == 1)


def test_a_half_mask_truncates_to_zero_and_the_crop_copies_the_window():
    sample = crop_sample(16, 16, (8.0, 8.0), mask_value=0.5)
    one, g = crop_both_ways(sample)
    assert g["dst"] == (0, 16, 0, 16) and g["src0"] == (0, 0)
    assert np.array_equal(one["image"], sample["image"])
    assert one["mask"].dtype == np.uint8 and np.all(one["mask"] == 0)
    sample = crop_sample(30, 30, (20.0, 25.0))                           # window rows 17..29 + 3 pad rows, columns 12..27
    one, _ = crop_both_ways(sample)
    assert np.array_equal(one["image"][:13], sample["image"][17:30, 12:28]) and np.all(one["image"][13:] == np.array(PAD, np.uint8))
    assert one["label"]["objpos"] == [8.0, 8.0] and one["label"]["keypoints"][0][:2] == [1.0 - 12, 2.0 - 17]


def test_plan_batch_refuses_what_it_cannot_run():
    t = T.CropPad(pad=PAD)
    s = crop_sample(16, 16, (8.0, 8.0))
    with pytest.raises(ValueError, match="order"):
        T.plan_batch([s], [T.Flip(), t])
    with pytest.raises(ValueError, match="CropPad"):
        T.plan_batch([s], [T.Flip()])
    with pytest.raises(ValueError, match="no samples"):
        T.plan_batch([], [t])
    big = crop_sample(16, 16, (8.0, 8.0))
    big["label"]["scale_provided"] = 0.6 / 4096                          # 16 * 4096 = 65536 >= 32768
    with pytest.raises(ValueError, match="32767"):
        T.plan_batch([big], [T.Scale(prob=0), t])


# ------------------------------------------------------------------------------------------ 3. pixel routines, by hand
def test_unit_scale_returns_the_input():
    g = np.random.default_rng(3)
    img = g.integers(0, 256, size=(13, 17, 3), dtype=np.uint8)
    m = g.random((13, 17), dtype=np.float32)
    assert np.array_equal(T.resize_linear(img, 1.0), img) and np.array_equal(T.resize_linear(m, 1.0), m)


def test_integer_translation_is_an_exact_shift_with_border_fill():
    g = np.random.default_rng(4)
    img = g.integers(0, 256, size=(11, 14, 3), dtype=np.uint8)
    m = g.random((11, 14), dtype=np.float32)
    R = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0]])                    # dst(x, y) = src(x - 3, y + 2)
    out, om = T.warp_affine(img, R, (16, 12), (7, 8, 9)), T.warp_affine(m, R, (16, 12), 1)
    exp = np.empty((12, 16, 3), np.uint8)
    exp[:] = np.array((7, 8, 9), np.uint8)
    exp[0:9, 3:16] = img[2:11, 0:13]
    em = np.ones((12, 16), np.float32)
    em[0:9, 3:16] = m[2:11, 0:13]
    assert out.dtype == np.uint8 and np.array_equal(out, exp)
    assert om.dtype == np.float32 and np.array_equal(om, em)


@pytest.mark.parametrize("degrees", [-40.0, -13.7, 0.0, 1.0, 29.3, 40.0, 90.0])
def test_an_all_ones_mask_stays_exactly_one(degrees):
    m = np.ones((23, 31), dtype=np.float32)
    up = T.resize_linear(m, 1.37)
    assert np.all(up == 1)
    R = T.rotation_matrix((up.shape[1] / 2, up.shape[0] / 2), degrees)
    assert np.all(T.warp_affine(up, R, (up.shape[1] + 5, up.shape[0] + 3), 1) == 1)


@pytest.mark.parametrize("h,w,s", [(7, 9, 1.9), (19, 23, 0.73), (30, 17, 6.0), (12, 40, 0.31), (5, 5, 3.3)])
def test_uint8_resize_is_within_one_grey_level_of_real_bilinear(h, w, s):
    """The bound, from the fixed-point steps (real bilinear at the SAME clamped taps and float32 fractions):
      - each 11-bit weight is off by at most 1/2 of 1/2048, and the pair still sums to 2048, so a pass is off by at most
        255 / 4096 = 0.0623 grey levels; two passes: +-0.125;
      - ``>> 4`` floors the row value in units of 16 / 2048 = 1/128 level: (-0.0079, 0];
      - ``>> 16`` floors each of the two products in units of 1/4 level: (-0.5, 0] together;
      - ``(.. + 2) >> 2`` rounds a multiple of 1/4 to the nearest level: [-0.25, +0.5].
    Lower end -0.125 - 0.0079 - 0.5 - 0.25 = -0.883, upper end +0.125 + 0.5 = +0.625: below 1, so the bound is 1."""
    g = np.random.default_rng(h * 1000 + w)
    img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    got = T.resize_linear(img, s).astype(np.float64)
    dh, dw = T.resized_dims(h, w, s)
    y0, y1, fy = T._linear_taps(dh, h, 1.0 / s)
    x0, x1, fx = T._linear_taps(dw, w, 1.0 / s)
    S, fx, fy = img.astype(np.float64), fx.astype(np.float64)[None, :, None], fy.astype(np.float64)[:, None, None]
    rows = S[:, x0] * (1 - fx) + S[:, x1] * fx
    real = rows[y0] * (1 - fy) + rows[y1] * fy
    worst = float(np.abs(got - real).max())
    print("worst deviation %.3f grey levels" % worst)
    assert got.shape == (dh, dw, 3) and worst <= 1.0


def test_the_warp_weights_sum_to_32768():
    j, i = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    w = T.warp_weights_u8(j, i)
    assert np.all(sum(w) == 32768) and all(np.all(v >= 0) for v in w)


def test_half_scale_is_the_two_by_two_area_average():
    g = np.random.default_rng(6)
    img = g.integers(0, 256, size=(8, 12, 3), dtype=np.uint8)
    m = g.random((8, 12), dtype=np.float32)
    S = img.astype(np.int64)
    exp = (S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2
    assert np.array_equal(T.resize_linear(img, 0.5), exp.astype(np.uint8))
    em = (((m[0::2, 0::2] + m[0::2, 1::2]) + m[1::2, 0::2]) + m[1::2, 1::2]) * np.float32(0.25)
    assert np.array_equal(T.resize_linear(m, 0.5), em)
    assert T.is_area_scale(1 / 0.5) and not T.is_area_scale(1 / 0.5000001)
    odd = T.resize_linear(img[:7, :7], 0.5)                              # rint(3.5) = 4: the last block repeats the last row / column
    assert odd.shape == (4, 4, 3) and odd[3, 3, 0] == img[6, 6, 0]


def test_the_small_mask_rounds_half_to_even():
    m = np.zeros((3, 8, 8), dtype=np.uint8)
    for n, ones in enumerate((31, 32, 33)):
        m[n].reshape(-1)[:ones] = 1
    small = T.mask_small_u8(m, 8)
    assert small.dtype == np.float32 and small.reshape(-1).tolist() == [0.0, 0.0, 1.0]
    assert T.mask_small_u8(np.ones((16, 24), np.uint8), 8).tolist() == [[1.0] * 3] * 2
    with pytest.raises(ValueError, match="blocks"):
        T.mask_small_u8(np.ones((16, 20), np.uint8), 8)


def test_rotation_matrix_and_its_inverse():
    R = T.rotation_matrix((10.0, 6.0), 90.0)
    assert np.allclose(R, [[0, 1, 4], [-1, 0, 16]], atol=1e-12)
    R = T.rotation_matrix((7.5, 11.0), 23.0)
    M = T.invert_affine(R).reshape(2, 3)
    full = np.vstack([R, [0, 0, 1]]) @ np.vstack([M, [0, 0, 1]])
    assert np.allclose(full, np.eye(3), atol=1e-12)
    assert np.array_equal(T.invert_affine([[0, 0, 1], [0, 0, 2]]), [0, 0, 0, 0, 0, 0])     # a singular matrix: D = 0


def test_oversized_intermediates_are_refused():
    with pytest.raises(ValueError, match="32767"):
        T.resize_linear(np.zeros((4, 4096, 3), np.uint8), 8.0)
    with pytest.raises(ValueError, match="32767"):
        T.warp_affine(np.zeros((4, 4), np.float32), np.eye(2, 3), (32768, 4), 1)


# ------------------------------------------------------------------------------------------ 4. the exports' argument checks
def good_plans(n=1):
    img = np.zeros((6, 5, 3), np.uint8)
    recs = (_lib.AugmentPlan * n)()
    for r in recs:
        r.image, r.mask, r.mem, r.rs_scale = img.ctypes.data, None, _lib.MEM_HOST, 1.0
        r.m[0], r.m[4] = 1.0, 1.0
        r.src_h, r.src_w, r.rs_h, r.rs_w, r.bound_h, r.bound_w = 6, 5, 6, 5, 6, 5
        r.should_crop, r.dst_y0, r.dst_y1, r.dst_x0, r.dst_x1 = 1, 0, 6, 0, 5
    return recs, img


def test_augment_exports_check_their_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.lwp_version() >= 103
    out = (C.c_float * 4096)()
    ms = C.c_float()

    def call(recs, N=1, ch=8, cw=16, stride=8, outs=(out, out, out)):
        return L.lwp_augment_batch(None, recs, N, ch, cw, stride, *outs), L.lwp_last_error(None)
    recs, img = good_plans()
    assert C.sizeof(_lib.AugmentPlan) == 144
    rc, msg = call(recs)
    assert rc == _lib.LWP_ERR_ARG and b"handle" in msg                   # everything else was accepted
    assert call(None)[0] == _lib.LWP_ERR_ARG and call(recs, outs=(out, None, out))[0] == _lib.LWP_ERR_ARG
    for N in (0, 65536):
        rc, msg = call(recs, N=N)
        assert rc == _lib.LWP_ERR_ARG and b"65535" in msg
    rc, msg = call(recs, ch=12)
    assert rc == _lib.LWP_ERR_ARG and b"blocks" in msg
    rc, msg = call(recs, ch=32768, stride=1)
    assert rc == _lib.LWP_ERR_ARG and b"32767" in msg
    assert call(recs, stride=0)[0] == _lib.LWP_ERR_ARG

    def broken(**fields):
        r, keep = good_plans()
        for k, v in fields.items():
            setattr(r[0], k, v)
        rc, msg = call(r)
        assert rc == _lib.LWP_ERR_ARG and b"sample 0" in msg, (fields, msg)
        return msg
    assert b"null" in broken(image=None)
    assert b"mem" in broken(mem=2)
    for name in ("src_h", "src_w", "rs_h", "rs_w", "bound_h", "bound_w"):
        assert b"32767" in broken(**{name: 32768}) and b"32767" in broken(**{name: 0})
    assert b"rs_scale" in broken(rs_scale=0.0) and b"rs_scale" in broken(rs_scale=float("inf"))
    assert b"0 or 1" in broken(flip=2) and b"0 or 1" in broken(area=-1)
    assert b"outside the crop" in broken(dst_y1=9) and b"outside the crop" in broken(dst_x0=-1)
    assert b"outside the bound" in broken(img_y0=1) and b"outside the bound" in broken(img_x0=-1)
    r, keep = good_plans()
    r[0].m[2] = float("nan")
    assert call(r)[0] == _lib.LWP_ERR_ARG and b"finite" in L.lwp_last_error(None)
    recs2, keep2 = good_plans(2)
    recs2[1].image = None
    rc, msg = call(recs2, N=2)
    assert rc == _lib.LWP_ERR_ARG and b"sample 1" in msg
    assert L.lwp_time_augment_batch(None, recs, 1, 8, 16, 8, out, out, out, 0, C.byref(ms)) == _lib.LWP_ERR_ARG
    assert L.lwp_time_augment_batch(None, recs, 1, 8, 16, 8, out, out, out, 3, C.byref(ms)) == _lib.LWP_ERR_ARG and b"handle" in L.lwp_last_error(None)


# ------------------------------------------------------------------------------------------ 5. the branch cases
# augment_branch_cases.py: what each batch is, and that it reaches the kernel path it is named for
def same_as_closed_form(b, result):
    """Every sample of the batch that has a closed form equals it in (image, mask) of ``result``; returns how many had one."""
    n_closed = 0
    for n, exp in enumerate(bc.closed_form(b)):
        if exp is None:
            continue
        n_closed += 1
        assert np.array_equal(result[0][n], ac.network_image(exp[0])), (b["name"], n)
        assert np.array_equal(result[1][n], exp[1]), (b["name"], n)
    return n_closed


def test_area_batches_plan_the_area_branch_with_and_without_the_clamp():
    b = bc.area_batch()
    plan, want = bc.plan_of(b), bc.host_result("area")
    assert [(g["src_h"], g["src_w"]) for g in plan.records[::3]] == list(bc.AREA_SOURCES)
    assert [(g["rs_h"], g["rs_w"]) for g in plan.records[::3]] == [(20, 28), (18, 26), (1, 1), (2, 2)]
    for n, g in enumerate(plan.records):
        assert g["scale"] == 0.5 and g["area"] is True and g["should_crop"]
        assert (plan.masks[n] is None) == (b["kinds"][n] == "none")
    assert {bool(g["flip"]) for g in plan.records[:6]} == {False, True}  # both flips among the samples that show picture
    shown = bc.picture(want[0]).reshape(len(plan), -1).mean(axis=1)
    assert np.all(shown[:6] >= 0.5), shown                               # 39 x 55 and 36 x 52: at least half the crop is picture
    for n in range(6):
        if b["kinds"][n] != "none":
            assert np.any(want[1][n] == 0) and np.any(want[1][n] == 1)
    fractions = b["samples"][0]["mask"]
    assert np.any((fractions > 0) & (fractions < 1))


def test_the_area_closed_form_holds_on_the_host_route():
    b = bc.area_closed_batch()
    plan, want = bc.plan_of(b), bc.host_result("area_closed")
    for n, g in enumerate(plan.records):
        assert g["scale"] == 0.5 and g["area"] is True and (g["rs_h"], g["rs_w"]) == (20, 28) and not g["flip"]
        assert g["dst"] == (10, 30, 22, 50) and g["src0"] == (0, 0)
        image, mask = bc.area_closed_expected(b["samples"][n])
        assert np.array_equal(image[10:30, 22:50], T.resize_linear(b["samples"][n]["image"], 0.5))
        outside = np.ones((40, 72), dtype=bool)
        outside[10:30, 22:50] = False
        assert np.all(image[outside] == np.array(bc.CROP_PAD, np.uint8)) and np.all(mask[outside] == 1)
    assert same_as_closed_form(b, want) == 2
    assert np.any(want[1][0] == 0) and np.any(want[1][0][10:30, 22:50] == 1) and np.all(want[1][1] == 1)


@pytest.mark.parametrize("name", ["area", "area_closed", "area_crowd_decoded"])
def test_the_bilinear_branch_at_a_step_of_two_gives_the_area_average(name, monkeypatch):
    """uint8: every weight is 1024, so >> 4, >> 16 and (.. + 2) >> 2 reduce to (a + b + c + d + 2) >> 2; a {0, 1} mask: every
    float operation is exact.  Fractional masks associate their sums differently and are left out."""
    b = bc.named(name)
    plan, want = bc.plan_of(b), bc.host_result(name)
    assert all(g["area"] is False for g in bc.with_area(plan, False).records) and all(g["area"] is True for g in plan.records)
    monkeypatch.setattr(T, "is_area_scale", lambda scale: False)
    linear = T.apply_plan_host(plan, b["stride"])
    exact = [n for n, kind in enumerate(b["kinds"]) if kind != "float"]
    assert len(exact) >= 2
    for n in exact:
        for got, exp in zip(linear, want):
            assert np.array_equal(got[n], exp[n]), (name, n)


def test_the_area_crowd_sample_equals_its_decoded_float_mask():
    with_segs, decoded = bc.area_crowd_batches()
    plan, plan_decoded = bc.plan_of(with_segs), bc.plan_of(decoded)
    assert [bool(s) for s in plan.segmentations] == [False, True, False] and plan.masks[1] is None and plan.crowd_runs is not None
    assert plan_decoded.segmentations is None and all(g["area"] for g in plan.records)
    want, want_decoded = bc.host_result("area_crowd"), bc.host_result("area_crowd_decoded")
    assert all(np.array_equal(a, d) for a, d in zip(want, want_decoded))
    assert 0 < int((want[1][1] == 0).sum()) < want[1][1].size and np.any(want[2][1] == 0)


def test_the_nothing_to_copy_batch_is_what_it_claims():
    b = bc.nothing_batch()
    plan, want = bc.plan_of(b), bc.host_result("nothing")
    g = plan.records
    assert [r["should_crop"] for r in g] == [True, False, True, True, True, True, True]
    assert g[3]["dst"] == (0, 0, 0, 16) and g[4]["dst"] == (0, 16, 16, 16) and g[5]["dst"] == (0, 13, 0, 16) and g[5]["src0"] == (17, 12)
    assert np.all(b["samples"][1]["mask"] == 0)                          # and it must not show
    assert all(int(s["image"].max()) < 100 for s in b["samples"])        # never a pad value in all three channels
    assert same_as_closed_form(b, want) == 7
    pad = ((np.array(bc.CROP_PAD, np.float32) - 128) / 256).reshape(3, 1, 1)
    for n in bc.NOTHING_ALL_PAD:
        assert np.all(want[0][n] == pad) and np.all(want[1][n] == 1) and np.all(want[2][n] == 1)
    assert np.all(want[1][5][:13] == 0) and np.all(want[1][5][13:] == 1) and np.all(want[2][5] == 0)


def test_the_identity_batches_plan_the_identity_warp_and_copy_the_window():
    for b in bc.identity_batches():
        plan, want = bc.plan_of(b), bc.host_result(b["name"])
        flipped = b["name"] == "identity_unit_scale_flipped"
        for g in plan.records:
            assert g["scale"] == 1.0 and not g["area"] and (g["rs_h"], g["rs_w"]) == (g["bound_h"], g["bound_w"]) == (30, 41)
            assert np.array_equal(g["minv"], [1, 0, 0, 0, 1, 0]) and bool(g["flip"]) == flipped
        assert [g["dst"] + g["src0"] for g in plan.records] == [(0, 16, 0, 18, 2, 23), (0, 11, 7, 24, 19, 0)]
        assert same_as_closed_form(b, want) == 2
        assert all(np.any(want[1][n] == 0) and np.any(want[1][n] == 1) for n in range(2))
        assert set(np.unique(b["samples"][0]["mask"]).tolist()) == {0.0, 0.5, 1.0}
    plain, mirrored = bc.host_result("identity_crop_only"), bc.host_result("identity_unit_scale_flipped")
    assert np.array_equal(mirrored[0], plain[0][..., ::-1]) and np.array_equal(mirrored[1], plain[1][..., ::-1])
    assert not np.array_equal(mirrored[1], plain[1])


@pytest.mark.parametrize("stride", bc.STRIDES)
def test_the_small_mask_batches_hold_ties_that_only_round_half_even_gets_right(stride):
    b = bc.small_mask_batch(stride)
    plan = bc.plan_of(b)
    image, mask, small = bc.host_result(b["name"])
    assert plan.crop_hw == bc.SMALL_CROP and b["stride"] == stride
    assert [g["dst"] + g["src0"] for g in plan.records] == [(0, 144, 0, 192, 3, 4), (0, 144, 0, 192, 5, 7), (52, 92, 71, 121, 0, 0)]
    assert np.array_equal(mask[0], bc.band_mask(stride, 1).astype(np.uint8))          # the design arrives in crop coordinates
    assert float(bc.picture(image)[2].mean()) < 0.1                      # mostly pad
    hs, ws = 144 // stride, 192 // stride
    assert small.shape == (3, hs, ws) and {4: 1728, 8: 432, 16: 108, 24: 48}[stride] == hs * ws
    ties, sums = bc.tie_blocks(mask, stride)
    inv = np.float32(1.0 / (stride * stride))
    assert np.float32(stride * stride // 2) * inv == np.float32(0.5)     # the tie is exact in float32 at this stride
    half_up = np.floor(sums.astype(np.float32) * inv + np.float32(0.5)).astype(np.float32)
    print("stride %d: %d tie blocks of %d" % (stride, int(ties.sum()), ties.size))
    assert int(ties[0].sum()) > 0 and int(ties[1].sum()) > 0
    assert np.array_equal(half_up != small, ties) and np.all(small[ties] == 0)
    for n in range(2):
        assert np.any(small[n] == 0) and np.any(small[n] == 1)
        assert not np.array_equal(small[n].reshape(ws, hs).T, small[n])  # h and w exchanged is another array
        shifted = np.roll(mask[n], 1, axis=1)
        assert not np.array_equal(T.mask_small_u8(shifted, stride), small[n])


def test_the_one_pixel_sides_show_picture_and_the_single_pixel_survives():
    b = bc.thin_batch()
    plan, want = bc.plan_of(b), bc.host_result("thin")
    assert [(g["src_h"], g["src_w"], g["rs_h"], g["rs_w"]) for g in plan.records] == [(1, 1, 6, 6), (1, 7, 6, 42), (7, 1, 21, 3)]
    shown = bc.picture(want[0]).reshape(3, -1).sum(axis=1)
    print("picture pixels:", shown.tolist())
    assert np.all(shown > 0) and all(np.any(want[1][n] == 0) for n in range(3))
    inside = bc.one_pixel_interior(want[0][0])
    pixel = ((np.array(bc.ONE_PIXEL, np.float32) - 128) / 256).reshape(3, 1)
    assert int(inside.sum()) > 0 and np.all(want[0][0][:, inside] == pixel)


def test_the_branch_table_keeps_its_coverage():
    area, clamped, crops, empty_y, empty_x, identity, flips, kinds, strides, outputs, ties, sides = set(), set(), set(), 0, 0, 0, set(), set(), set(), set(), 0, set()
    names = []
    for b in bc.all_batches():
        names.append(b["name"])
        plan = bc.plan_of(b)
        strides.add(b["stride"])
        kinds.update(b["kinds"])
        outputs.add((plan.crop_hw[0] // b["stride"]) * (plan.crop_hw[1] // b["stride"]))
        if b["name"].startswith("small_mask"):
            ties += int(bc.tie_blocks(bc.host_result(b["name"])[1], b["stride"])[0].sum())
        for g in plan.records:
            area.add(g["area"])
            if g["area"]:
                clamped.add(2 * g["rs_h"] > g["src_h"] and 2 * g["rs_w"] > g["src_w"])
            crops.add(g["should_crop"])
            dy0, dy1, dx0, dx1 = g["dst"]
            empty_y += g["should_crop"] and dy0 == dy1 and dx0 < dx1
            empty_x += g["should_crop"] and dx0 == dx1 and dy0 < dy1
            identity += not any(isinstance(t, (T.Scale, T.Rotate)) for t in b["transforms"])
            flips.add(bool(g["flip"]))
            sides.add(min(g["src_h"], g["src_w"]))
    assert tuple(names) == bc.NAMES and len(set(names)) == len(names)
    assert area == {False, True} and clamped == {False, True} and crops == {False, True} and empty_y and empty_x and identity
    assert flips == {False, True} and kinds == {"none", "binary", "float", "segmentations"} and strides == set(bc.STRIDES)
    assert any(n > 256 and n % 256 for n in outputs) and ties > 0 and 1 in sides
    assert {b["route"] for b in bc.all_batches()} == {"plan", "samples", "device_augment"}
