"""CPU: crowd masks from uncompressed RLE (datasets.coco.get_mask / pack_crowd_runs, the segmentation input of plan_batch and
apply_plan_host) and the argument checks of lwp_crowd_masks, lwp_time_crowd_masks and lwp_augment_batch_crowd, which need no
GPU.  The oracle is the loop restatement of crowd_mask_cases.py, pinned here to the two examples of maskApi.h's own comment
and to hand-written grids; it is unpinned against pycocotools itself."""
import copy
import ctypes as C
import random

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.datasets import coco
from lwpose_amd.datasets import transformations as T

import augment_cases as ac
import crowd_mask_cases as cm

NAMES = list(cm.CASES)


# ------------------------------------------------------------------------------------------ 1. the restatement's pins
def transposed_decode(counts, h, w):
    """The runs laid out row by row."""
    return cm.rle_decode(counts, h, w).reshape(-1, order="F").reshape(h, w)


HAND = [
    # maskApi.h: M = [0 0 1 1 1 0 1] -> [2 3 1 1]; M = [1 1 1 1 1 1 0] -> [0 6 1]
    ([2, 3, 1, 1], 7, 1, [[0], [0], [1], [1], [1], [0], [1]]),
    ([0, 6, 1], 7, 1, [[1], [1], [1], [1], [1], [1], [0]]),
    ([2, 3, 1, 1], 1, 7, [[0, 0, 1, 1, 1, 0, 1]]),
    # positions 0..5 = 0 1 1 0 0 1, laid out column by column
    ([1, 2, 2, 1], 3, 2, [[0, 0], [1, 0], [1, 1]]),
    ([1, 2, 2, 1], 2, 3, [[0, 1, 0], [1, 0, 1]]),
    # a zero-length run in the middle joins its neighbours; the tail past the last run is zeros
    ([1, 1, 0, 2], 3, 2, [[0, 1], [1, 0], [1, 0]]),
]


@pytest.mark.parametrize("counts,h,w,grid", HAND)
def test_the_restatement_decodes_the_closed_form_cases(counts, h, w, grid):
    grid = np.array(grid, dtype=np.uint8)
    assert np.array_equal(cm.rle_decode(counts, h, w), grid)
    assert np.array_equal(cm.search_decode(counts, h, w), grid)
    if sum(counts) == h * w and 0 not in counts[1:]:
        assert cm.rle_encode(grid) == {"counts": counts, "size": [h, w]}


def test_a_transposed_decode_fails_the_hand_written_grids():
    for counts, h, w, grid in HAND[3:5]:
        assert not np.array_equal(transposed_decode(counts, h, w), np.array(grid))
        assert not np.array_equal(cm.search_decode(counts, h, w, row_major=True), np.array(grid))


def test_the_encoder_round_trips():
    for seed, (h, w) in enumerate([(1, 1), (5, 3), (3, 5), (17, 9)]):
        grid = cm.blob_grid(h, w, seed)
        enc = cm.rle_encode(grid)
        assert sum(enc["counts"]) == h * w and np.array_equal(cm.rle_decode(enc["counts"], h, w), grid)
    assert cm.rle_encode(np.ones((2, 2), dtype=bool))["counts"] == [0, 4]


# ------------------------------------------------------------------------------------------ 2. get_mask, pack_crowd_runs
@pytest.mark.parametrize("name", NAMES)
def test_get_mask_equals_the_restatement_in_place(name):
    sizes, segs, want = cm.case(name)
    for hw, s, w in zip(sizes, segs, want):
        mask = np.ones(hw, dtype=np.float32)
        before = copy.deepcopy(s)
        out = coco.get_mask(s, mask)
        assert out is mask and s == before
        assert mask.dtype == np.float32 and np.array_equal(mask, w)
        for seg in s:                                  # the kernel's statement of the decode agrees with the loop
            assert np.array_equal(cm.search_decode(seg["counts"], *hw), cm.rle_decode(seg["counts"], *hw))


def test_get_mask_keeps_what_the_mask_held():
    mask = np.full((4, 3), 0.25, dtype=np.float32)
    coco.get_mask([cm.rle([0, 5, 7], 4, 3)], mask)
    assert mask.T.reshape(-1).tolist() == [0.0] * 5 + [0.25] * 7


def test_the_table_holds_what_it_is_meant_to():
    assert any(np.all(w == 0) for w in cm.case("all_ones")[2]) and all(np.all(w == 1) for w in cm.case("all_zeros")[2])
    sizes, segs, want = cm.case("short_tail")
    assert want[0].T.reshape(-1)[14:].tolist() == [1.0] * 16
    for name, n in (("lds_exact", cm.LDS_RUNS), ("lds_plus_one", cm.LDS_RUNS + 1), ("lds_two_segments_exact", cm.LDS_RUNS),
                    ("lds_two_segments_plus_one", cm.LDS_RUNS + 1)):
        sizes, segs, want = cm.case(name)
        assert sum(len(s["counts"]) for s in segs[0]) == n
        assert 0 < int((want[0] == 0).sum()) < want[0].size
    assert cm.case("empty_between")[1][1] == [] and np.all(cm.case("empty_between")[2][1] == 1)
    u = cm.case("three_overlapping")
    single = [cm.get_mask_ref([s], np.ones(u[0][0], dtype=np.float32)) for s in u[1][0]]
    assert all(int((m == 0).sum()) < int((u[2][0] == 0).sum()) for m in single)        # no one segmentation is the union


@pytest.mark.parametrize("name", NAMES)
def test_pack_crowd_runs_round_trips(name):
    sizes, segs, _ = cm.case(name)
    counts, seg_off, image_seg_off = coco.pack_crowd_runs(segs, sizes)
    assert counts.dtype == seg_off.dtype == image_seg_off.dtype == np.int64
    assert len(image_seg_off) == len(sizes) + 1 and image_seg_off[0] == 0 and seg_off[0] == 0 and seg_off[-1] == len(counts)
    back = [[{"counts": counts[seg_off[s]:seg_off[s + 1]].tolist(), "size": list(hw)}
             for s in range(image_seg_off[n], image_seg_off[n + 1])] for n, hw in enumerate(sizes)]
    assert back == [[{"counts": list(s["counts"]), "size": list(s["size"])} for s in ss] for ss in segs]
    assert coco.pack_crowd_runs([None] + segs, [(2, 2)] + sizes)[2].tolist() == [0] + image_seg_off.tolist()


BAD = [
    ("size", cm.rle([2, 2], 2, 3)),                    # the dict of a 2 x 3 image on a 3 x 2 one
    ("sum", cm.rle([3, 4], 3, 2)),
    ("negative", cm.rle([2, -1, 3], 3, 2)),
    ("integer", cm.rle([2, 1.5], 3, 2)),
    ("integer", cm.rle([2, "3"], 3, 2)),
    ("sum", cm.rle([2, 2 ** 70], 3, 2)),
    ("compressed", {"counts": "52203", "size": [3, 2]}),
    ("compressed", {"counts": b"52203", "size": [3, 2]}),
    ("RLE dict", [[0, 0, 1, 0, 1, 1]]),                # polygons
    ("RLE dict", [0, 0, 2, 2]),                        # a box
    ("RLE dict", {"counts": [6]}),
]


@pytest.mark.parametrize("word,seg", BAD)
def test_what_is_out_of_scope_is_a_value_error_that_names_the_sample(word, seg):
    good = cm.rle([1, 2], 3, 2)
    mask = np.ones((3, 2), dtype=np.float32)
    with pytest.raises(ValueError, match=word) as e:
        coco.get_mask([good, seg], mask)
    assert "segmentation 1" in str(e.value) and np.all(mask == 1)        # nothing was written
    with pytest.raises(ValueError, match=word) as e:
        coco.pack_crowd_runs([[good], [], [good, good, seg]], [(3, 2)] * 3)
    assert "sample 2, segmentation 2" in str(e.value)
    sample = ac.synthetic_sample(1, 3, 2, with_mask=False)
    sample["segmentations"] = [seg]
    ok = dict(ac.synthetic_sample(2, 3, 2, with_mask=False), segmentations=[good])
    with pytest.raises(ValueError, match=word) as e:
        T.plan_batch([ok, sample], [T.CropPad(pad=(0, 0, 0), crop_x=8, crop_y=8)], random.Random(0))
    assert "sample 1" in str(e.value)


def test_numpy_integer_counts_are_integers():
    seg = {"counts": np.array([1, 2, 3], dtype=np.int32), "size": (3, 2)}
    assert np.array_equal(coco.get_mask([seg], np.ones((3, 2), np.float32)), cm.get_mask_ref([cm.rle([1, 2, 3], 3, 2)], np.ones((3, 2), np.float32)))
    with pytest.raises(ValueError, match="2 lists"):
        coco.pack_crowd_runs([[], []], [(3, 2)])


# ------------------------------------------------------------------------------------------ 3. the C entries without a GPU
def i64(*v):
    return (C.c_int64 * len(v))(*v)


def i32(*v):
    return (C.c_int * len(v))(*v)


def crowd_call(counts=(2, 3, 1), seg_off=(0, 3), image_seg_off=(0, 1), heights=(3,), widths=(2,), N=1, out_off=(0, 6), masks=True,
               timed=None):
    L = _lib.lib()
    buf = (C.c_float * 64)()
    args = [None, i64(*counts) if counts else None, seg_off and i64(*seg_off), image_seg_off and i64(*image_seg_off),
            heights and i32(*heights), widths and i32(*widths), N, out_off and i64(*out_off), buf if masks else None]
    if timed is not None:
        ms = C.c_float()
        return L.lwp_time_crowd_masks(*args, timed, C.byref(ms)), L.lwp_last_error(None)
    return L.lwp_crowd_masks(*args), L.lwp_last_error(None)


def test_crowd_masks_argument_checks_need_no_gpu():
    E = _lib.LWP_ERR_ARG
    rc, msg = crowd_call()
    assert rc == E and b"handle" in msg                                  # everything else was accepted
    rc, msg = crowd_call(counts=(), seg_off=(0, 0))                     # a segmentation without a count; counts may then be NULL
    assert rc == E and b"handle" in msg
    for missing in ("seg_off", "image_seg_off", "heights", "widths", "out_off"):
        rc, msg = crowd_call(**{missing: None})
        assert rc == E and b"null" in msg, missing
    assert crowd_call(masks=False)[0] == E and b"null" in crowd_call(masks=False)[1]
    rc, msg = crowd_call(counts=None)
    assert rc == E and b"counts is null" in msg
    for N in (0, -1, 65536):
        rc, msg = crowd_call(N=N)
        assert rc == E and b"65535" in msg
    two = dict(N=2, heights=(3, 3), widths=(2, 2), out_off=(0, 6, 12))
    for kw, word in ((dict(image_seg_off=(1, 1, 1)), b"start at 0"), (dict(seg_off=(1, 3)), b"start at 0"),
                     (dict(out_off=(1, 7, 13)), b"start at 0")):
        rc, msg = crowd_call(**dict(dict(two, image_seg_off=(0, 0, 1)), **kw))
        assert rc == E and word in msg, kw
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 1, 0)))
    assert rc == E and b"sample 1" in msg and b"descends" in msg
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 1, 2), seg_off=(0, 3, 2)))
    assert rc == E and b"sample 1" in msg and b"descends" in msg
    for bad in ((0, 2), (3, 0), (32768, 2), (3, 32768)):
        rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), heights=(3, bad[0]), widths=(2, bad[1])))
        assert rc == E and b"sample 1" in msg and b"32767" in msg, bad
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), counts=(2, 3, 2)))
    assert rc == E and b"sample 1" in msg and b"sum" in msg
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), counts=(2, 2 ** 62, 2 ** 62)))     # the sum is taken in 64 bits
    assert rc == E and b"sample 1" in msg and b"sum" in msg
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), counts=(2, -1, 3)))
    assert rc == E and b"sample 1" in msg and b"negative" in msg
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), out_off=(0, 6, 11)))
    assert rc == E and b"sample 1" in msg and b"out_off" in msg
    rc, msg = crowd_call(**dict(two, image_seg_off=(0, 0, 1), out_off=(0, 8, 14)))               # gaps are the caller's business
    assert rc == E and b"handle" in msg
    assert crowd_call(timed=0)[0] == E
    rc, msg = crowd_call(timed=3)
    assert rc == E and b"handle" in msg
    rc, msg = crowd_call(timed=3, counts=(2, 3, 2))
    assert rc == E and b"sum" in msg


def augment_crowd_call(masks=(None, None), counts=(2, 3, 1), seg_off=(0, 3), image_seg_off=(0, 0, 1), N=2):
    L = _lib.lib()
    img = np.zeros((3, 2, 3), dtype=np.uint8)
    flt = np.ones((3, 2), dtype=np.float32)
    recs = (_lib.AugmentPlan * 2)()
    for r, m in zip(recs, masks):
        r.image, r.mask, r.mem, r.rs_scale = img.ctypes.data, (flt.ctypes.data if m else None), _lib.MEM_HOST, 1.0
        r.m[0], r.m[4] = 1.0, 1.0
        r.src_h, r.src_w, r.rs_h, r.rs_w, r.bound_h, r.bound_w = 3, 2, 3, 2, 3, 2
    out = (C.c_float * 1024)()
    rc = L.lwp_augment_batch_crowd(None, recs, N, 8, 16, 8, i64(*counts) if counts else None, seg_off and i64(*seg_off),
                                   image_seg_off and i64(*image_seg_off), out, out, out)
    return rc, L.lwp_last_error(None)


def test_augment_batch_crowd_argument_checks_need_no_gpu():
    E = _lib.LWP_ERR_ARG
    rc, msg = augment_crowd_call()
    assert rc == E and b"handle" in msg
    rc, msg = augment_crowd_call(masks=(True, None))                     # a float mask on a sample WITHOUT segmentations is fine
    assert rc == E and b"handle" in msg
    rc, msg = augment_crowd_call(masks=(None, True))
    assert rc == E and b"sample 1" in msg and b"null mask" in msg
    rc, msg = augment_crowd_call(counts=(2, 3, 2))                       # the size is the plan's src_h x src_w
    assert rc == E and b"sample 1" in msg and b"sum" in msg
    for missing in ("seg_off", "image_seg_off"):
        rc, msg = augment_crowd_call(**{missing: None})
        assert rc == E and b"null" in msg
    rc, msg = augment_crowd_call(image_seg_off=(0, 1, 0))
    assert rc == E and b"sample 1" in msg
    rc, msg = augment_crowd_call(N=0)
    assert rc == E and b"65535" in msg


# ------------------------------------------------------------------------------------------ 4. the augmentation's host half
def segmentation_samples():
    """(samples that carry segmentations / None / [], the same samples with the decoded float mask / None / None)."""
    with_segs, with_masks = [], []
    for n in range(6):
        h, w = 14 + 3 * n, 31 - 2 * n
        s = ac.synthetic_sample(700 + n, h, w, others=n % 2, scale_provided=0.3, with_mask=False)
        del s["mask"]
        segs = None if n % 3 == 1 else [] if n % 3 == 2 else [cm.rle_encode(cm.blob_grid(h, w, 50 + n)), cm.rle([h, 2 * h + 1, 3], h, w)]
        with_segs.append(dict(s, segmentations=segs))
        with_masks.append(dict(s, mask=cm.get_mask_ref(segs, np.ones((h, w), dtype=np.float32)) if segs else None))
    return with_segs, with_masks


def test_plan_batch_and_the_host_path_take_segmentations():
    with_segs, with_masks = segmentation_samples()
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=(128, 128, 128)),
                  T.CropPad(pad=(1, 2, 3), center_perterb_max=6, crop_x=32, crop_y=24), T.Flip()]
    before = copy.deepcopy([s["segmentations"] for s in with_segs])
    a = T.plan_batch(with_segs, transforms, random.Random(5))
    b = T.plan_batch(with_masks, transforms, random.Random(5))
    assert [s["segmentations"] for s in with_segs] == before
    assert a.segmentations == before and all(m is None for m in a.masks) and b.segmentations is None
    assert a.records[0].keys() == b.records[0].keys() and np.array_equal(a.kpts, b.kpts)
    got, want = T.apply_plan_host(a, 8), T.apply_plan_host(b, 8)
    assert int((want[1] == 0).sum()) > 0                                 # the crowd regions reach the crops
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    with pytest.raises(ValueError, match="sample 0 carries both"):
        T.plan_batch([dict(with_masks[0], segmentations=[])], transforms, random.Random(5))
    positional = T.BatchPlan(b.records, b.images, b.masks, b.labels, b.crop_hw)          # the signature from before
    assert positional.segmentations is None


# ------------------------------------------------------------------------------------------ 5. the labels the feature consumes
def test_prepare_train_labels_returns_what_the_reference_script_did():
    """tests/golden/prepare_train_labels.json (tools/make_crowd_golden.py): a synthetic annotation file and the list the
    reference's own script wrote for it.  Values, types and order; and the segmentations it hands on decode."""
    import json
    import os
    from conftest import GOLDEN
    from lwpose_amd.scripts import prepare_train_labels as P
    with open(os.path.join(GOLDEN, "prepare_train_labels.json")) as f:
        fx = json.load(f)
    data = copy.deepcopy(fx["data"])
    got = P.prepare(data, fx["net_input_size"])
    assert data == fx["data"]                                            # the annotations are not modified
    assert got == fx["expected"]
    assert json.dumps(got, sort_keys=True) == json.dumps(fx["expected"], sort_keys=True)         # ints stay ints, floats floats
    assert [g["image_id"] for g in got] == [11, 11, 23, 8]
    assert [len(g["segmentations"]) for g in got] == [1, 1, 2, 0]        # the crowd of the image without people went with it
    assert [len(g["processed_other_annotations"]) for g in got] == [4, 4, 0, 1]
    for g in got:
        mask = coco.get_mask(g["segmentations"], np.ones((g["img_height"], g["img_width"]), dtype=np.float32))
        want = cm.get_mask_ref(g["segmentations"], np.ones(mask.shape, dtype=np.float32))
        assert np.array_equal(mask, want) and bool(np.any(mask == 0)) == bool(g["segmentations"])
    per_image = {11: [[a for a in fx["data"]["annotations"] if a["image_id"] == 11 and not a["iscrowd"]], []]}
    info = {i["id"]: i for i in fx["data"]["images"]}
    direct = P.prepare_annotations(per_image, info, fx["net_input_size"])
    assert [dict(d, segmentations=got[0]["segmentations"]) for d in direct] == got[:2]


# ------------------------------------------------------------------------------------------ 6. the oracle can fail
def masks_with(decode=cm.rle_decode, only_last=False):
    out = {}
    for name in NAMES:
        sizes, segs, _ = cm.case(name)
        out[name] = [cm.get_mask_ref(s, np.ones(hw, dtype=np.float32), decode, only_last) for hw, s in zip(sizes, segs)]
    return out


def failing(masks):
    return [n for n in NAMES if not all(np.array_equal(a, b) for a, b in zip(masks[n], cm.case(n)[2]))]


def test_mutated_oracles_fail_the_case_table():
    assert failing(masks_with()) == []
    assert failing(masks_with(cm.search_decode)) == []
    lower = failing(masks_with(lambda c, h, w: cm.search_decode(c, h, w, side="left")))
    rows = failing(masks_with(lambda c, h, w: cm.search_decode(c, h, w, row_major=True)))
    last = failing(masks_with(only_last=True))
    assert lower and rows and last
    assert "5x3" in rows and "3x5" in rows and "1xW" not in rows and "Hx1" not in rows
    assert set(last) >= {"three_overlapping", "zero_runs_middle"}
    assert "zero_runs_middle" in lower and "leading_zero" in lower
