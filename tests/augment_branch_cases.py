"""Shared by test_augment_host.py and test_gpu_augment.py: batches built to reach the paths of csrc/augment_kernels.hip that
the recorded fixtures and random draws never take — the 2 x 2 area branch, should_crop == 0 and an empty window, the identity
warp, the small mask past one workgroup at four strides with round-half-even ties, and sources one pixel wide or high.

A batch is a dict: ``name``, ``samples`` (host arrays, fresh at every call of its builder), ``transforms``, ``seed`` (of the
random.Random handed to plan_batch), ``stride``, ``route`` (which entry point the GPU test drives: "plan" is
Engine.augment_batch(plan), "samples" Engine.augment_batch(samples, transforms, rng), "device_augment" DeviceAugment) and
``kinds`` (per sample, what its mask is: "none", "binary", "float" or "segmentations").  Every batch keeps the two pad colours
apart (WARP_PAD, CROP_PAD), so a swap of them shows.  Nothing here needs a GPU."""
import random

import numpy as np

from lwpose_amd.datasets import transformations as T

import augment_cases as ac
import crowd_mask_cases as cm

WARP_PAD, CROP_PAD = (128, 128, 128), (1, 2, 3)
STRIDES = (4, 8, 16, 24)
_F32 = np.float32


def batch(name, samples, transforms, seed, kinds, stride=8, route="plan"):
    assert len(kinds) == len(samples)
    return {"name": name, "samples": samples, "transforms": transforms, "seed": seed, "kinds": list(kinds), "stride": stride,
            "route": route}


def plan_of(b, samples=None):
    return T.plan_batch(b["samples"] if samples is None else samples, b["transforms"], random.Random(b["seed"]))


def with_area(plan, area):
    """The same plan with every record's ``area`` forced: False sends a source step of exactly 2 down the bilinear branch."""
    return T.BatchPlan([dict(g, area=bool(area)) for g in plan.records], plan.images, plan.masks, plan.labels, plan.crop_hw,
                       plan.segmentations)


def is_pad(image_nchw, pad):
    """(N, H, W) bool: all three channels of the network image hold the pad colour."""
    v = ((np.asarray(pad, dtype=np.float32) - _F32(128)) / _F32(256)).reshape(1, 3, 1, 1)
    return np.all(image_nchw == v, axis=1)


def picture(image_nchw):
    """(N, H, W) bool: neither pad colour (pixels blended with the warp pad count as picture)."""
    return ~is_pad(image_nchw, CROP_PAD) & ~is_pad(image_nchw, WARP_PAD)


def full_list(scale_prob=0, max_rotate_degree=40, center_perterb_max=4, crop_x=32, crop_y=24, flip_prob=0.5):
    return [T.ConvertKeypoints(), T.Scale(prob=scale_prob), T.Rotate(pad=WARP_PAD, max_rotate_degree=max_rotate_degree),
            T.CropPad(pad=CROP_PAD, center_perterb_max=center_perterb_max, crop_x=crop_x, crop_y=crop_y), T.Flip(prob=flip_prob)]


def mask_of(kind, h, w, seed):
    """None, a {0, 1} mask or one with fractions; the lower left quarter is all ones, so that 1 survives the averaging."""
    if kind == "none":
        return None
    g = np.random.default_rng(seed)
    m = (g.random((h, w)) < 0.7).astype(_F32) if kind == "binary" else g.random((h, w), dtype=_F32)
    m[h // 2:, :max(w // 2, 1)] = 1
    return m


# ---------------------------------------------------------------------------------------------- A. the area branch
AREA_SOURCES = ((39, 55), (36, 52), (2, 2), (3, 3))       # 39 x 55: rint(19.5), rint(27.5) round up, the last taps clamp at n - 1
AREA_SCALE_PROVIDED = 1.2                                 # 0.6 / 1.2 == 0.5 exactly


def area_sample(seed, h, w, kind):
    s = ac.synthetic_sample(seed, h, w, others=1, scale_provided=AREA_SCALE_PROVIDED, with_mask=False)
    s["mask"] = mask_of(kind, h, w, seed + 1000)
    return s


def area_batch():
    """Every source with a fractional, a binary and no mask; Scale(prob=0), Rotate at +-40 degrees, crop 24 x 32, Flip."""
    samples, kinds = [], []
    for k, (h, w) in enumerate(AREA_SOURCES):
        for j, kind in enumerate(("float", "binary", "none")):
            samples.append(area_sample(4100 + 10 * k + j, h, w, kind))
            kinds.append(kind)
    return batch("area", samples, full_list(), 11, kinds)


def area_closed_batch():
    """The 39 x 55 source, no rotation, no flip, no jitter, objpos at the centre, crop 40 x 72: the whole 20 x 28 average lies
    inside the crop at rows 10..29, columns 22..49."""
    samples, kinds = [], ("binary", "none")
    for j, kind in enumerate(kinds):
        s = area_sample(4200 + j, 39, 55, kind)
        s["label"]["objpos"] = [27.5, 19.5]
        samples.append(s)
    return batch("area_closed", samples, full_list(max_rotate_degree=0, center_perterb_max=0, crop_x=72, crop_y=40, flip_prob=0), 12,
                 kinds)


def area_closed_expected(sample):
    """(uint8 (40, 72, 3) image, uint8 (40, 72) mask) of a sample of area_closed_batch, from the source alone: the 2 x 2
    average (a + b + c + d + 2) >> 2 with the last row and column repeated; a binary mask keeps 1 where all four are 1."""
    src = sample["image"].astype(np.int64)
    src = np.concatenate([src, src[-1:]], axis=0)
    src = np.concatenate([src, src[:, -1:]], axis=1)                     # 40 x 56: the odd row and column repeated
    avg = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + 2) >> 2
    image = np.empty((40, 72, 3), np.uint8)
    image[:] = np.array(CROP_PAD, np.uint8)
    image[10:30, 22:50] = avg
    mask = np.ones((40, 72), np.uint8)
    if sample["mask"] is not None:
        m = np.pad(sample["mask"], ((0, 1), (0, 1)), mode="edge")
        mask[10:30, 22:50] = (m[0::2, 0::2] + m[0::2, 1::2] + m[1::2, 0::2] + m[1::2, 1::2]) == 4
    return image, mask


def area_crowd_batches():
    """(with segmentations, with the decoded float mask): three 36 x 52 area samples, the middle one a crowd rectangle."""
    grid = np.zeros((36, 52), dtype=bool)
    grid[7:22, 11:40] = True
    seg = cm.rle_encode(grid)
    with_segs = [area_sample(4300, 36, 52, "binary"), area_sample(4301, 36, 52, "none"), area_sample(4302, 36, 52, "none")]
    with_masks = [area_sample(4300, 36, 52, "binary"), area_sample(4301, 36, 52, "none"), area_sample(4302, 36, 52, "none")]
    with_segs[1]["segmentations"] = [seg]
    with_masks[1]["mask"] = cm.get_mask_ref([seg], np.ones((36, 52), dtype=np.float32))
    return (batch("area_crowd", with_segs, full_list(), 13, ("binary", "segmentations", "none")),
            batch("area_crowd_decoded", with_masks, full_list(), 13, ("binary", "binary", "none")))


# ---------------------------------------------------------------------------------------------- B. nothing to copy
def nothing_batch():
    """CropPad alone, crop 16 x 16: [ordinary, should_crop False (its mask of zeros must not show), ordinary, a window empty
    in y, one empty in x, a window of 13 rows over a mask of 0.5, ordinary]."""
    samples = [ac.crop_sample(16, 16, (8.0, 8.0)),
               ac.crop_sample(60, 20, (10.0, 38.0), mask_value=0.0),     # y_start = 30 >= w = 20
               ac.crop_sample(40, 40, (20.0, 20.0)),
               ac.crop_sample(20, 60, (30.0, 28.0)),                     # y_start = 20 == h
               ac.crop_sample(20, 60, (-8.0, 10.0)),                     # x_start = -16, x_finish = 0
               ac.crop_sample(30, 30, (20.0, 25.0), mask_value=0.5),     # rows 17..29, columns 12..27, then 3 pad rows
               ac.crop_sample(23, 31, (14.0, 12.0))]
    return batch("nothing", samples, [T.CropPad(pad=CROP_PAD, center_perterb_max=0, crop_x=16, crop_y=16)], 14, ["float"] * 7,
                 route="samples")


NOTHING_ALL_PAD = (1, 3, 4)                               # the samples of nothing_batch with no picture at all


def nothing_expected(b):
    """Per sample (uint8 (16, 16, 3) image, uint8 (16, 16) mask) as slices of the source."""
    s = b["samples"]
    pad = np.empty((16, 16, 3), np.uint8)
    pad[:] = np.array(CROP_PAD, np.uint8)
    ones = np.ones((16, 16), np.uint8)
    window, window_mask = pad.copy(), ones.copy()
    window[:13] = s[5]["image"][17:30, 12:28]
    window_mask[:13] = 0                                                 # 0.5 truncates to 0
    return [(s[0]["image"], ones), (pad, ones), (s[2]["image"][12:28, 12:28], ones), (pad, ones), (pad, ones), (window, window_mask),
            (s[6]["image"][4:20, 6:22], ones)]


# ---------------------------------------------------------------------------------------------- C. identity warp
def _identity_samples(scale_provided):
    g = np.random.default_rng(43)
    samples = [ac.crop_sample(30, 41, (35.0, 10.0), seed=4400), ac.crop_sample(30, 41, (5.0, 27.0), seed=4401)]
    for s in samples:
        s["mask"] = g.integers(0, 3, size=(30, 41)).astype(_F32) * _F32(0.5)      # 0, 0.5 and 1: only 1 survives the crop
        s["label"]["scale_provided"] = scale_provided
    return samples


def identity_batches():
    """Crop 16 x 24 of two 30 x 41 sources under three transform lists that all plan the identity warp."""
    crop = lambda: T.CropPad(pad=CROP_PAD, center_perterb_max=0, crop_x=24, crop_y=16)
    lists = (("identity_crop_only", [crop()]),
             ("identity_unit_scale_flipped", [T.Scale(prob=0), crop(), T.Flip(prob=1)]),
             ("identity_zero_rotation", [T.Rotate(pad=WARP_PAD, max_rotate_degree=0), crop()]))
    return [batch(name, _identity_samples(0.6), tr, 15 + k, ("float", "float"), route="device_augment") for k, (name, tr) in enumerate(lists)]


def identity_expected(b):
    """Per sample (uint8 (16, 24, 3) image, uint8 (16, 24) mask), as slices of the source: objpos (35, 10) puts source rows
    2..17, columns 23..40 at crop columns 0..17; objpos (5, 27) puts rows 19..29, columns 0..16 at crop rows 0..10, columns
    7..23.  A list with Flip(prob=1) mirrors both."""
    out = []
    for s, (dy0, dy1, dx0, dx1, sy0, sy1, sx0, sx1) in zip(b["samples"], ((0, 16, 0, 18, 2, 18, 23, 41), (0, 11, 7, 24, 19, 30, 0, 17))):
        image = np.empty((16, 24, 3), np.uint8)
        image[:] = np.array(CROP_PAD, np.uint8)
        mask = np.ones((16, 24), np.uint8)
        image[dy0:dy1, dx0:dx1] = s["image"][sy0:sy1, sx0:sx1]
        mask[dy0:dy1, dx0:dx1] = s["mask"][sy0:sy1, sx0:sx1] == 1
        if any(isinstance(t, T.Flip) for t in b["transforms"]):
            image, mask = image[:, ::-1], mask[:, ::-1]
        out.append((np.ascontiguousarray(image), np.ascontiguousarray(mask)))
    return out


# ---------------------------------------------------------------------------------------------- D. the small mask
SMALL_CROP = (144, 192)                                   # a multiple of 4, 8, 16 and 24, and not square


def band_mask(stride, seed):
    """A {0, 1} mask in crop coordinates whose block rows cycle through six bands: the left half of every block 0 (the block
    sums to stride^2 / 2: a tie), the same with one more 1 (rounds to 1), with one fewer (rounds to 0), columns of 1 and 0 one
    pixel wide, random bits, all ones."""
    h, w = SMALL_CROP
    y, x = np.mgrid[0:h, 0:w]
    band = (y // stride) % 6
    first = y % stride == 0
    m = np.where(x % stride >= stride // 2, 1, 0)
    m[(band == 1) & first & (x % stride == 0)] = 1
    m[(band == 2) & first & (x % stride == stride // 2)] = 0
    m = np.where(band == 3, x % 2, m)
    m = np.where(band == 4, np.random.default_rng(seed).integers(0, 2, size=(h, w)), m)
    m = np.where(band == 5, 1, m)
    return m.astype(_F32)


def small_mask_batch(stride):
    """CropPad alone, crop 144 x 192: two 150 x 200 sources whose crop is a plain window (origins (3, 4) and (5, 7)) and a
    40 x 50 source that lands at crop rows 52..91, columns 71..120; the band mask of ``stride`` mapped back into each."""
    a, b, c = ac.crop_sample(150, 200, (100.0, 75.0), seed=4500), ac.crop_sample(150, 200, (103.5, 77.0), seed=4501), \
        ac.crop_sample(40, 50, (25.0, 20.0), seed=4502)
    g = np.random.default_rng(4503)
    for s, (y0, x0), seed in ((a, (3, 4), 1), (b, (5, 7), 2)):
        s["mask"] = g.integers(0, 2, size=(150, 200)).astype(_F32)        # random outside the window: a shifted read shows
        s["mask"][y0:y0 + 144, x0:x0 + 192] = band_mask(stride, seed)
    c["mask"] = np.ascontiguousarray(band_mask(stride, 3)[52:92, 71:121])
    return batch("small_mask_stride_%d" % stride, [a, b, c], [T.CropPad(pad=CROP_PAD, center_perterb_max=0, crop_x=192, crop_y=144)],
                 16, ("binary",) * 3, stride=stride)


def tie_blocks(mask_u8, stride):
    """(…, H // stride, W // stride) bool: the block holds exactly stride^2 / 2 ones."""
    H, W = mask_u8.shape[-2:]
    sums = mask_u8.reshape(mask_u8.shape[:-2] + (H // stride, stride, W // stride, stride)).astype(np.int64).sum(axis=(-3, -1))
    return sums * 2 == stride * stride, sums


# ---------------------------------------------------------------------------------------------- E. one-pixel sides
ONE_PIXEL = (200, 40, 90)                                 # the 1 x 1 source: apart from both pads in every channel


def thin_batch():
    """1 x 1 (enlarged to 6 x 6), 1 x 7 (6 x 42) and 7 x 1 (21 x 3) sources, the full list, crop 16 x 24, objpos at the
    centre of the source so that each crop shows picture."""
    samples, g = [], np.random.default_rng(46)
    for k, (h, w, sp) in enumerate(((1, 1, 0.1), (1, 7, 0.1), (7, 1, 0.2))):
        s = ac.synthetic_sample(4600 + k, h, w, others=k % 2, scale_provided=sp, with_mask=False)
        s["label"]["objpos"] = [w / 2, h / 2]
        samples.append(s)
    samples[0]["image"][:] = np.array(ONE_PIXEL, np.uint8)
    samples[0]["mask"] = np.zeros((1, 1), dtype=_F32)                    # 0 inside and where it blends with the border's 1
    samples[1]["mask"] = g.integers(0, 2, size=(1, 7)).astype(_F32)
    samples[2]["mask"] = np.maximum(g.random((7, 1), dtype=_F32), (np.arange(7) % 3 == 0).astype(_F32)[:, None])
    return batch("thin", samples, full_list(crop_x=24, crop_y=16), 17, ("binary", "binary", "float"))


def erode(region):
    """(H, W) bool: the pixel and its eight neighbours all lie in the region (the frame does not)."""
    p = np.pad(region, 1, constant_values=False)
    out = np.ones_like(region)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + region.shape[0], dx:dx + region.shape[1]]
    return out


def one_pixel_interior(image_chw):
    """The pixels of the 1 x 1 case whose 3 x 3 neighbourhood holds neither pad colour.  The enlarged source is a 6 x 6
    square of ONE_PIXEL; the warp blends it with WARP_PAD where a tap falls off it, a ring about one pixel wide, and is
    WARP_PAD beyond.  A step to one of the eight neighbours moves |cos| + |sin| >= 1 pixels along the square's normal, so a
    pixel of the ring has a neighbour past it, and what is left after the erosion took all four taps from the square."""
    return erode(picture(image_chw[None])[0])


# ---------------------------------------------------------------------------------------------- the table
def all_batches():
    with_segs, decoded = area_crowd_batches()
    return ([area_batch(), area_closed_batch(), with_segs, decoded, nothing_batch()] + identity_batches() +
            [small_mask_batch(s) for s in STRIDES] + [thin_batch()])


NAMES = ("area", "area_closed", "area_crowd", "area_crowd_decoded", "nothing", "identity_crop_only", "identity_unit_scale_flipped",
         "identity_zero_rotation") + tuple("small_mask_stride_%d" % s for s in STRIDES) + ("thin",)


def named(name):
    """The batch of that name, fresh."""
    return {b["name"]: b for b in all_batches()}[name]


def closed_form(b):
    """Per sample (uint8 (H, W, 3) image, uint8 (H, W) mask) where the result follows from the source by slices and the 2 x 2
    average alone, without the staged route; None elsewhere."""
    if b["name"] == "area_closed":
        return [area_closed_expected(s) for s in b["samples"]]
    if b["name"] == "nothing":
        return nothing_expected(b)
    if b["name"].startswith("identity"):
        return identity_expected(b)
    return [None] * len(b["samples"])


_HOST = {}


def host_result(name):
    """(image, mask, mask_small) of T.apply_plan_host over the named batch at its stride: computed once, shared, read only."""
    if name not in _HOST:
        b = named(name)
        _HOST[name] = T.apply_plan_host(plan_of(b), b["stride"])
        for a in _HOST[name]:
            a.setflags(write=False)
    return _HOST[name]
