"""Drop-in for the reference's ``datasets.transformations`` (train.py:33-38): ``ConvertKeypoints -> Scale -> Rotate ->
CropPad -> Flip``, as five classes that work on one sample in NumPy, and as a batch plan whose pixels one kernel launch
renders on the GPU (``DeviceAugment``; csrc/augment_kernels.hip).

A sample is ``{"image": uint8 (H, W, 3), "mask": float32 (H, W) with values in [0, 1] or None (all ones), "label": a dict in
scripts/prepare_train_labels.py's format}``.  Every transform is split in two: ``plan(hw, label, rng)`` draws its random
numbers, moves the label exactly as the reference's Python does (same statements, same order, float64) and returns the
geometry; the pixel half applies that geometry with the three routines below.  ``__call__`` does both; ``plan_batch`` runs
only the first half per sample and hands the geometry to the device.

The pixel routines restate OpenCV's plain C path (``resize_linear``, ``rotation_matrix``, ``warp_affine``); cv2 is not a
dependency and they are NOT pinned against it.  Mask values must lie in [0, 1]; this is not checked.
"""
import copy
import math
import random

import numpy as np

from .coco import _rle_counts, get_mask, labels_to_arrays, pack_crowd_runs

MAX_DIM = 32768                      # OpenCV's remap coordinates saturate to short there: refused instead
_F32 = np.float32


def _check_dims(*dims):
    for d in dims:
        if not 1 <= int(d) < MAX_DIM:
            raise ValueError("an image dimension of %d is outside 1..%d" % (int(d), MAX_DIM - 1))


# ---------------------------------------------------------------------------------------------- pixel routines
def _linear_taps(n_dst, n_src, scale):
    """Per destination index of one axis: the two clamped source indices and the float32 weight of the second."""
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(_F32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(_F32)
    low, high = i < 0, i >= n_src - 1
    i[low], f[low] = 0, 0
    i[high], f[high] = n_src - 1, 0
    return i, np.minimum(i + 1, n_src - 1), f


def resized_dims(h, w, s):
    """(dh, dw) of cv2.resize(dsize=(0, 0), fx=s, fy=s): round-half-even of the scaled size."""
    return int(np.rint(h * s)), int(np.rint(w * s))


def is_area_scale(scale):
    """True where OpenCV swaps INTER_LINEAR for the 2 x 2 area average: the source step is 2 to within DBL_EPSILON."""
    return abs(scale - 2.0) < np.finfo(np.float64).eps


def resize_linear(src, s):
    """cv2.resize(src, dsize=(0, 0), fx=s, fy=s) with INTER_LINEAR for a uint8 (H, W[, C]) image (11-bit fixed-point
    weights, two passes) or a float32 (H, W) mask.  At s = 0.5 it is the 2 x 2 block average; a block that hangs over the
    last row or column repeats it."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    dh, dw = resized_dims(h, w, s)
    _check_dims(h, w, dh, dw)
    scale = 1.0 / s
    is_u8 = src.dtype == np.uint8
    if not is_u8 and src.dtype != np.float32:
        raise TypeError("resize_linear takes uint8 or float32, got %s" % src.dtype)
    if is_area_scale(scale):
        y0, x0 = np.minimum(2 * np.arange(dh), h - 1), np.minimum(2 * np.arange(dw), w - 1)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        S = src.astype(np.int32) if is_u8 else src
        p00, p01, p10, p11 = S[y0][:, x0], S[y0][:, x1], S[y1][:, x0], S[y1][:, x1]
        if is_u8:
            return ((p00 + p01 + p10 + p11 + 2) >> 2).astype(np.uint8)
        return (((p00 + p01) + p10) + p11) * _F32(0.25)
    y0, y1, fy = _linear_taps(dh, h, scale)
    x0, x1, fx = _linear_taps(dw, w, scale)
    tail = (1,) * (src.ndim - 2)
    if is_u8:
        a1 = np.rint(fx * _F32(2048)).astype(np.int32).reshape((1, dw) + tail)
        a0 = np.rint((_F32(1) - fx) * _F32(2048)).astype(np.int32).reshape((1, dw) + tail)
        b1 = np.rint(fy * _F32(2048)).astype(np.int32).reshape((dh, 1) + tail)
        b0 = np.rint((_F32(1) - fy) * _F32(2048)).astype(np.int32).reshape((dh, 1) + tail)
        S = src.astype(np.int32)
        rows = (S[:, x0] * a0 + S[:, x1] * a1) >> 4
        out = (((b0 * rows[y0]) >> 16) + ((b1 * rows[y1]) >> 16) + 2) >> 2
        return out.astype(np.uint8)
    fx = fx.reshape((1, dw) + tail)
    fy = fy.reshape((dh, 1) + tail)
    rows = src[:, x0] * (_F32(1) - fx) + src[:, x1] * fx
    return rows[y0] * (_F32(1) - fy) + rows[y1] * fy


def rotation_matrix(center, degrees, scale=1.0):
    """cv2.getRotationMatrix2D: the 2 x 3 float64 matrix of a rotation by ``degrees`` (counter-clockwise, the y axis
    pointing down) about ``center`` = (cx, cy)."""
    a = degrees * math.pi / 180
    alpha, beta = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = center
    return np.array([[alpha, beta, (1 - alpha) * cx - beta * cy],
                     [-beta, alpha, beta * cx + (1 - alpha) * cy]], dtype=np.float64)


def invert_affine(R):
    """The destination -> source matrix cv2.warpAffine derives from R, as six float64 values, statement by statement."""
    M = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return np.array(M, dtype=np.float64)


def warp_coords(minv, bound_h, bound_w):
    """The 5-bit fixed-point source coordinates of every destination pixel: integer parts (sy, sx) and the 1/32 fractions
    (j, i), each (bound_h, bound_w) int64."""
    M = [float(v) for v in minv]
    x = np.arange(bound_w, dtype=np.float64)
    y = np.arange(bound_h, dtype=np.float64)
    X = ((np.rint((M[1] * y + M[2]) * 1024).astype(np.int64) + 16)[:, None] + np.rint(M[0] * x * 1024).astype(np.int64)[None, :]) >> 5
    Y = ((np.rint((M[4] * y + M[5]) * 1024).astype(np.int64) + 16)[:, None] + np.rint(M[3] * x * 1024).astype(np.int64)[None, :]) >> 5
    return Y >> 5, X >> 5, Y & 31, X & 31


def warp_weights_u8(j, i):
    """The four 15-bit integer weights of the taps (sy, sx), (sy, sx+1), (sy+1, sx), (sy+1, sx+1); they sum to 32768."""
    return 32 * (32 - i) * (32 - j), 32 * i * (32 - j), 32 * (32 - i) * j, 32 * i * j


def warp_affine(src, R, dsize, border, inverse=False):
    """cv2.warpAffine(src, R, dsize=(width, height), INTER_LINEAR, BORDER_CONSTANT, borderValue=border) for a uint8
    (H, W[, C]) image or a float32 (H, W) mask.  ``border``: a scalar, or one value per channel.  With ``inverse`` R is
    already the six values of ``invert_affine``."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    bound_w, bound_h = int(dsize[0]), int(dsize[1])
    _check_dims(h, w, bound_h, bound_w)
    minv = np.asarray(R, dtype=np.float64).reshape(6) if inverse else invert_affine(R)
    sy, sx, j, i = warp_coords(minv, bound_h, bound_w)
    is_u8 = src.dtype == np.uint8
    if not is_u8 and src.dtype != np.float32:
        raise TypeError("warp_affine takes uint8 or float32, got %s" % src.dtype)
    work = np.int32 if is_u8 else np.float32             # 255 * 32768 + 2^14 < 2^31
    fill = np.broadcast_to(np.asarray(border, dtype=work), src.shape[2:])
    S = src.astype(work)

    def tap(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = S[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
        return np.where(inside.reshape(inside.shape + (1,) * (src.ndim - 2)), v, fill)
    p0, p1, p2, p3 = tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)
    ext = lambda a: a.reshape(a.shape + (1,) * (src.ndim - 2))
    if is_u8:
        w0, w1, w2, w3 = (ext(v.astype(np.int32)) for v in warp_weights_u8(j, i))
        return ((p0 * w0 + p1 * w1 + p2 * w2 + p3 * w3 + (1 << 14)) >> 15).astype(np.uint8)
    vx1, vy1 = i.astype(_F32) / _F32(32), j.astype(_F32) / _F32(32)
    vx0, vy0 = _F32(1) - vx1, _F32(1) - vy1
    return ((p0 * ext(vy0 * vx0) + p1 * ext(vy0 * vx1)) + p2 * ext(vy1 * vx0)) + p3 * ext(vy1 * vx1)


def flip_horizontal(src):
    """cv2.flip(src, 1)."""
    return np.ascontiguousarray(np.asarray(src)[:, ::-1])


def mask_small_u8(mask, stride):
    """coco.py:48 on the uint8 mask CropPad leaves: cv2.resize(mask, fx = fy = 1 / stride, INTER_AREA) of a uint8 image is
    rint(float32(block sum) * float32(1 / stride^2)), round-half-even.  (…, H, W) uint8 -> (…, H // stride, W // stride)
    float32; H and W must be multiples of the stride."""
    m = np.asarray(mask)
    H, W = m.shape[-2:]
    if H % stride or W % stride:
        raise ValueError("a %d x %d mask is not a whole number of %d x %d blocks" % (H, W, stride, stride))
    sums = m.reshape(m.shape[:-2] + (H // stride, stride, W // stride, stride)).astype(np.int64).sum(axis=(-3, -1))
    return np.rint(sums.astype(_F32) * _F32(1.0 / (stride * stride))).astype(_F32)


# ---------------------------------------------------------------------------------------------- the five transforms
def _people(label):
    return [label] + list(label["processed_other_annotations"])


def _ones_mask(sample):
    if sample.get("mask") is None:
        sample["mask"] = np.ones(sample["image"].shape[:2], dtype=np.float32)
    return sample["mask"]


class ConvertKeypoints:
    """COCO's 17 key-points -> the network's 18 (the neck between the shoulders), visibility 2 for what lies at (0, 0) or
    outside the ORIGINAL frame."""
    _ORDER = (0, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3)        # source row of every output row but the neck

    def plan(self, hw, label, rng=random):
        h, w = hw
        for person in _people(label):
            for kp in person["keypoints"]:
                if kp[0] == kp[1] == 0:
                    kp[2] = 2
                if kp[0] < 0 or kp[0] >= w or kp[1] < 0 or kp[1] >= h:
                    kp[2] = 2
        for person in _people(label):
            person["keypoints"] = self._convert(person["keypoints"], w, h)
        return {}

    def _convert(self, kps, w, h):
        left, right = kps[5], kps[6]
        neck = [(left[0] + right[0]) / 2, (left[1] + right[1]) / 2, 0]
        if left[2] == 2 or right[2] == 2:
            neck[2] = 2
        elif left[2] == 1 and right[2] == 1:
            neck[2] = 1
        if neck[0] < 0 or neck[0] >= w or neck[1] < 0 or neck[1] >= h:
            neck[2] = 2
        out = [kps[i] for i in self._ORDER]
        out.insert(1, neck)
        return out

    def __call__(self, sample):
        self.plan(sample["image"].shape[:2], sample["label"])
        return sample


class Scale:
    def __init__(self, prob=1, min_scale=0.5, max_scale=1.1, target_dist=0.6):
        self._prob, self._min_scale, self._max_scale, self._target_dist = prob, min_scale, max_scale, target_dist

    def plan(self, hw, label, rng=random):
        multiplier = 1
        if rng.random() <= self._prob:
            multiplier = (self._max_scale - self._min_scale) * rng.random() + self._min_scale
        scale = self._target_dist / label["scale_provided"] * multiplier
        dh, dw = resized_dims(hw[0], hw[1], scale)
        _check_dims(hw[0], hw[1], dh, dw)
        label["img_height"], label["img_width"] = dh, dw
        label["objpos"][0] *= scale
        label["objpos"][1] *= scale
        for kp in label["keypoints"]:
            kp[0] *= scale
            kp[1] *= scale
        for other in label["processed_other_annotations"]:
            other["objpos"][0] *= scale
            other["objpos"][1] *= scale
            for kp in other["keypoints"]:
                kp[0] *= scale
                kp[1] *= scale
        return {"scale": scale, "rs_h": dh, "rs_w": dw}

    def __call__(self, sample):
        mask = _ones_mask(sample)
        g = self.plan(sample["image"].shape[:2], sample["label"])
        sample["image"] = resize_linear(sample["image"], g["scale"])
        sample["mask"] = resize_linear(mask, g["scale"])
        return sample


class Rotate:
    def __init__(self, pad, max_rotate_degree=40):
        self._pad, self._max_rotate_degree = pad, max_rotate_degree

    def plan(self, hw, label, rng=random):
        degree = (rng.random() - 0.5) * 2 * self._max_rotate_degree
        h, w = hw
        center = (w / 2, h / 2)
        R = rotation_matrix(center, degree, 1)
        abs_cos, abs_sin = abs(R[0, 0]), abs(R[0, 1])
        bound_w = int(h * abs_sin + w * abs_cos)
        bound_h = int(h * abs_cos + w * abs_sin)
        _check_dims(bound_h, bound_w)
        R[0, 2] += bound_w / 2 - center[0]
        R[1, 2] += bound_h / 2 - center[1]
        label["img_height"], label["img_width"] = bound_h, bound_w
        label["objpos"] = self._rotate(label["objpos"], R)
        for person in _people(label):
            for kp in person["keypoints"]:
                kp[0], kp[1] = self._rotate(kp, R)
        return {"R": R, "bound_h": bound_h, "bound_w": bound_w, "warp_pad": tuple(self._pad)}

    @staticmethod
    def _rotate(p, R):
        return [R[0, 0] * p[0] + R[0, 1] * p[1] + R[0, 2], R[1, 0] * p[0] + R[1, 1] * p[1] + R[1, 2]]

    def __call__(self, sample):
        mask = _ones_mask(sample)
        g = self.plan(sample["image"].shape[:2], sample["label"])
        dsize = (g["bound_w"], g["bound_h"])
        sample["image"] = warp_affine(sample["image"], g["R"], dsize, g["warp_pad"])
        sample["mask"] = warp_affine(mask, g["R"], dsize, 1)
        return sample


def _copy_extent(dst_slice, dst_n, src_slice, src_n):
    """One axis of ``dst[a:b] = src[c:d]`` as NumPy resolves it: (dst start, dst stop, src start).  Unequal lengths are
    NumPy's ValueError.  (A length-1 source, which NumPy would broadcast, cannot arise while the label's size is the image's,
    as Scale and Rotate leave it; it is refused like any other mismatch.)"""
    d0, d1, _ = slice(*dst_slice).indices(dst_n)
    s0, s1, _ = slice(*src_slice).indices(src_n)
    dn, sn = max(d1 - d0, 0), max(s1 - s0, 0)
    if dn != sn:
        raise ValueError("could not broadcast input array from shape (%d,) into shape (%d,)" % (sn, dn))
    return d0, d0 + dn, s0


class CropPad:
    def __init__(self, pad, center_perterb_max=40, crop_x=368, crop_y=368):
        self._pad, self._center_perterb_max, self._crop_x, self._crop_y = pad, center_perterb_max, crop_x, crop_y

    def plan(self, hw, label, rng=random):
        prob_x = rng.random()
        prob_y = rng.random()
        cx, cy = self._crop_x, self._crop_y
        offset_x = int((prob_x - 0.5) * 2 * self._center_perterb_max)
        offset_y = int((prob_y - 0.5) * 2 * self._center_perterb_max)
        center = (label["objpos"][0] + offset_x, label["objpos"][1] + offset_y)
        x_start, y_start = int(center[0] - cx / 2), int(center[1] - cy / 2)
        offset_left, offset_up = -x_start, -y_start
        x_finish, y_finish = x_start + cx, y_start + cy
        dx_start, dy_start, dx_finish, dy_finish = 0, 0, cx, cy
        w, h = label["img_width"], label["img_height"]
        should_crop = True
        if x_start < 0:
            dx_start -= x_start
            x_start = 0
        if x_start >= w:
            should_crop = False
        if y_start < 0:
            dy_start -= y_start
            y_start = 0
        if y_start >= w:                               # the reference compares the row with the WIDTH: kept
            should_crop = False
        if x_finish > w:
            dx_finish -= x_finish - w
            x_finish = w
        if x_finish < 0:
            should_crop = False
        if y_finish > h:
            dy_finish -= y_finish - h
            y_finish = h
        if y_finish < 0:
            should_crop = False
        g = {"crop_h": cy, "crop_w": cx, "should_crop": should_crop, "crop_pad": tuple(self._pad),
             "dst": (0, 0, 0, 0), "src0": (0, 0)}
        if should_crop:                                # the slice assignment, resolved as NumPy would (it may raise)
            dy0, dy1, sy0 = _copy_extent((dy_start, dy_finish), cy, (y_start, y_finish), hw[0])
            dx0, dx1, sx0 = _copy_extent((dx_start, dx_finish), cx, (x_start, x_finish), hw[1])
            g.update(dst=(dy0, dy1, dx0, dx1), src0=(sy0, sx0))
        label["img_width"], label["img_height"] = cx, cy
        label["objpos"][0] += offset_left
        label["objpos"][1] += offset_up
        for person in _people(label):
            for kp in person["keypoints"]:
                kp[0] += offset_left
                kp[1] += offset_up
        return g

    @staticmethod
    def pixels(image, mask, g):
        """(uint8 crop, uint8 mask) of a warped image and its float32 mask: the mask is TRUNCATED to uint8 on assignment, as
        the reference's uint8 ``cropped_mask`` does, so only 1.0 survives."""
        out = np.empty((g["crop_h"], g["crop_w"], 3), dtype=np.uint8)
        out[:] = np.asarray(g["crop_pad"], dtype=np.uint8)
        out_mask = np.ones((g["crop_h"], g["crop_w"]), dtype=np.uint8)
        if g["should_crop"]:
            dy0, dy1, dx0, dx1 = g["dst"]
            sy0, sx0 = g["src0"]
            out[dy0:dy1, dx0:dx1] = image[sy0:sy0 + dy1 - dy0, sx0:sx0 + dx1 - dx0]
            out_mask[dy0:dy1, dx0:dx1] = mask[sy0:sy0 + dy1 - dy0, sx0:sx0 + dx1 - dx0]
        return out, out_mask

    def __call__(self, sample):
        mask = _ones_mask(sample)
        g = self.plan(sample["image"].shape[:2], sample["label"])
        sample["image"], sample["mask"] = self.pixels(sample["image"], mask, g)
        return sample


class Flip:
    _RIGHT = (2, 3, 4, 8, 9, 10, 14, 16)
    _LEFT = (5, 6, 7, 11, 12, 13, 15, 17)

    def __init__(self, prob=0.5):
        self._prob = prob

    def plan(self, hw, label, rng=random):
        if not rng.random() <= self._prob:
            return {"flip": False}
        w = label["img_width"]
        label["objpos"][0] = w - 1 - label["objpos"][0]
        for other in label["processed_other_annotations"]:
            other["objpos"][0] = w - 1 - other["objpos"][0]
        for person in _people(label):
            kps = person["keypoints"]
            for kp in kps:
                kp[0] = w - 1 - kp[0]
            for r, l in zip(self._RIGHT, self._LEFT):
                kps[r], kps[l] = kps[l], kps[r]
        return {"flip": True}

    def __call__(self, sample):
        mask = _ones_mask(sample)
        if self.plan(sample["image"].shape[:2], sample["label"])["flip"]:
            sample["image"] = flip_horizontal(sample["image"])
            sample["mask"] = flip_horizontal(mask)
        return sample


# ---------------------------------------------------------------------------------------------- batch plan
_ORDER = (ConvertKeypoints, Scale, Rotate, CropPad, Flip)


class BatchPlan(object):
    """What ``plan_batch`` returns.  ``records``: per sample the geometry dict (src_h, src_w, scale, rs_h, rs_w, rs_scale,
    area, minv (6 float64), bound_h, bound_w, warp_pad, crop_pad, should_crop, dst, src0, flip); ``images`` /
    ``masks``: the sources, untouched; ``labels``: the transformed label dicts; ``kpts`` (N, Pmax, 18, 3) float64 and
    ``n_persons`` (N,) int32 in ``labels_to_arrays``' layout; ``crop_hw``; ``segmentations``: per sample its list of crowd RLE
    dicts, or None where the sample came with a float mask or with neither (None for the whole batch: no sample has any);
    ``crowd_runs``: ``pack_crowd_runs`` of them, made at construction (None when no sample has a segmentation)."""

    def __init__(self, records, images, masks, labels, crop_hw, segmentations=None):
        self.records, self.images, self.masks, self.labels, self.crop_hw = records, images, masks, labels, crop_hw
        self.segmentations = segmentations
        self.crowd_runs = None                         # the arrays of the C call, packed once: the host half of the crowd masks
        if segmentations is not None and any(segmentations):
            self.crowd_runs = pack_crowd_runs(segmentations, [(g["src_h"], g["src_w"]) for g in records])
        self.kpts, self.n_persons = labels_to_arrays(labels)

    def __len__(self):
        return len(self.records)


def plan_batch(samples, transforms, rng=None):
    """The host half of a batch: per sample, in order, every transform's random draws (from ``rng.random()``; Python's global
    ``random`` when None), its label arithmetic and its geometry.  ``transforms``: instances of the five classes in the
    reference's order; ``CropPad`` is required (it fixes the output size), the others may be left out.  No pixel is touched
    and the samples are not modified (labels are deep-copied).  A sample whose crop the reference cannot assign raises
    ValueError here as it does there.  A sample may carry ``"segmentations"`` (a list of uncompressed RLE dicts, possibly
    empty: ``label['segmentations']``) instead of a float ``"mask"``: its mask is ``get_mask`` of all ones, decoded by
    ``apply_plan_host`` on the host and rendered by ``Engine.augment_batch`` on the device.  Both at once is a ValueError, and
    so is an RLE that ``get_mask`` refuses."""
    rng = random if rng is None else rng
    kinds = [type(t) for t in transforms]
    places = [_ORDER.index(k) if k in _ORDER else -1 for k in kinds]
    if -1 in places or any(b <= a for a, b in zip(places, places[1:])):
        raise ValueError("transforms must be ConvertKeypoints, Scale, Rotate, CropPad, Flip instances in that order, each at most once")
    if CropPad not in kinds:
        raise ValueError("a batch needs a CropPad: it fixes the size every sample ends with")
    if len(samples) == 0:
        raise ValueError("no samples")
    records, images, masks, labels, segmentations = [], [], [], [], []
    for n, sample in enumerate(samples):
        image, mask, segs = sample["image"], sample.get("mask"), sample.get("segmentations")
        if mask is not None and segs is not None:
            raise ValueError("sample %d carries both a mask and segmentations" % n)
        if len(image.shape) != 3 or image.shape[2] != 3:
            raise ValueError("expected an image of shape (H, W, 3), got %s" % (tuple(image.shape),))
        h, w = int(image.shape[0]), int(image.shape[1])
        if mask is not None and tuple(mask.shape) != (h, w):
            raise ValueError("a mask of shape %s does not belong to a %d x %d image" % (tuple(mask.shape), h, w))
        _check_dims(h, w)
        if segs is not None:
            segs = list(segs)
            for k, seg in enumerate(segs):             # the checks of get_mask, before anything is planned
                _rle_counts(seg, h, w, "sample %d, segmentation %d" % (n, k))
        segmentations.append(segs)
        label = copy.deepcopy(sample["label"])
        g = {"src_h": h, "src_w": w, "scale": 1.0, "rs_h": h, "rs_w": w, "R": None, "bound_h": None, "warp_pad": (0, 0, 0),
             "flip": False}
        hw = (h, w)
        for t in transforms:
            g.update(t.plan(hw, label, rng))
            if isinstance(t, Scale):
                hw = (g["rs_h"], g["rs_w"])
            elif isinstance(t, Rotate):
                hw = (g["bound_h"], g["bound_w"])
        if g["bound_h"] is None:                       # no Rotate: the identity warp of the resized image
            g["bound_h"], g["bound_w"] = g["rs_h"], g["rs_w"]
        g["rs_scale"] = 1.0 / g["scale"]
        g["area"] = bool(is_area_scale(g["rs_scale"]))
        g["minv"] = invert_affine(g["R"]) if g["R"] is not None else np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
        records.append(g)
        images.append(image)
        masks.append(mask)
        labels.append(label)
    crops = set((g["crop_h"], g["crop_w"]) for g in records)
    if all(segs is None for segs in segmentations):
        segmentations = None
    return BatchPlan(records, images, masks, labels, crops.pop(), segmentations)


def _to_numpy(a, dtype):
    if getattr(a, "is_cuda", False) or hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def apply_plan_host(plan, stride=8):
    """The staged NumPy route over a plan: resize, warp, crop and flip of every sample, each stage a full image, as the
    reference runs them.  Returns ``image`` (N, 3, cy, cx) float32 ((v - 128) / 256), ``mask`` (N, cy, cx) uint8 and
    ``mask_small`` (N, cy // stride, cx // stride) float32: the CPU path, and the oracle of the kernel."""
    cy, cx = plan.crop_hw
    image = np.empty((len(plan), 3, cy, cx), dtype=np.float32)
    mask = np.empty((len(plan), cy, cx), dtype=np.uint8)
    for n, g in enumerate(plan.records):
        img = _to_numpy(plan.images[n], np.uint8)
        m = np.ones(img.shape[:2], dtype=np.float32) if plan.masks[n] is None else _to_numpy(plan.masks[n], np.float32)
        if plan.segmentations is not None and plan.segmentations[n]:
            m = get_mask(plan.segmentations[n], m)
        img, m = resize_linear(img, g["scale"]), resize_linear(m, g["scale"])
        dsize = (g["bound_w"], g["bound_h"])
        img = warp_affine(img, g["minv"], dsize, g["warp_pad"], inverse=True)
        m = warp_affine(m, g["minv"], dsize, 1, inverse=True)
        img, m = CropPad.pixels(img, m, g)
        if g["flip"]:
            img, m = flip_horizontal(img), flip_horizontal(m)
        image[n] = ((img.astype(np.float32) - _F32(128)) / _F32(256)).transpose(2, 0, 1)
        mask[n] = m
    return image, mask, mask_small_u8(mask, stride)


class DeviceAugment(object):
    """The batched front end: ``DeviceAugment(transforms)(samples)`` turns N raw samples into what the training step
    consumes.  The host draws the random numbers and moves the labels (``plan_batch``); one kernel launch renders the
    N x 3 x cy x cx crops straight from the source images (``Engine.augment_batch``).  Sources may be NumPy arrays (packed
    and uploaded in one copy) or cuda uint8 / float32 tensors (read in place).  Returns a dict: ``image`` (N, 3, cy, cx)
    float32, ``mask`` (N, cy, cx) uint8, ``mask_small`` (N, cy // stride, cx // stride) float32 — cuda tensors — and
    ``kpts`` / ``n_persons`` (the arrays ``Engine.train_targets`` takes), ``labels`` and the ``plan``."""

    def __init__(self, transforms, engine=None, stride=8, rng=None):
        self.transforms, self.engine, self.stride, self.rng = list(transforms), engine, int(stride), rng

    def __call__(self, samples, engine=None):
        engine = self.engine if engine is None else engine
        if engine is None:
            raise ValueError("DeviceAugment needs an Engine (at construction or per call)")
        engine = getattr(engine, "engine", engine)
        plan = plan_batch(samples, self.transforms, self.rng)
        image, mask, mask_small, _ = engine.augment_batch(plan, stride=self.stride)
        return {"image": image, "mask": mask, "mask_small": mask_small, "kpts": plan.kpts, "n_persons": plan.n_persons,
                "labels": plan.labels, "plan": plan}
