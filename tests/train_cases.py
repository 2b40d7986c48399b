"""Training-target, mask and loss cases (plain data + deterministic builders) and their NumPy restatement in float64, shared by
tools/make_train_golden.py, tests/test_train_host.py, tests/test_gpu_train.py and tools/targets_bench.py.

The fixtures tests/golden/train_*.npz hold each case's inputs and what the reference's own statements made of them
(datasets/coco.py:71-159, modules/loss.py); ``targets`` / ``mask_mean`` / ``l2_loss64`` below restate them vectorised, and
tests/test_train_host.py pins the restatement to the fixtures.  ``targets_loops`` is the same thing as per-pixel Python loops,
the shape of the reference's code: tools/targets_bench.py times it."""
import math

import numpy as np

import skeleton_cases as sc

CHUNK = 8                     # persons the targets kernel stages at a time (csrc/lwp_internal.h kTrainChunk)

# coco.py:13-14's limb order: limb j owns PAF channels 2j, 2j + 1
COCO_TRAIN_LIMBS = [[1, 8], [8, 9], [9, 10], [1, 11], [11, 12], [12, 13], [1, 2], [2, 3], [3, 4], [2, 16],
                    [1, 5], [5, 6], [6, 7], [5, 17], [1, 0], [0, 14], [0, 15], [14, 16], [15, 17]]
# a standing person in a unit box (x right, y down), COCO order of the network's 18 key-points
_CANON18 = np.array([[.5, .08], [.5, .2], [.36, .2], [.3, .38], [.27, .54], [.64, .2], [.7, .38], [.73, .54], [.42, .52],
                     [.41, .74], [.4, .95], [.58, .52], [.59, .74], [.6, .95], [.46, .05], [.54, .05], [.41, .08], [.59, .08]])


def skeleton(name):
    """(K, limb_kpts, limb_pafs) as Engine.set_skeleton takes them; 'coco' is the engine's default table."""
    if name == "coco":
        return 18, [list(p) for p in sc.COCO_KPTS], [list(p) for p in sc.COCO_PAFS]
    if name == "hand21":
        return 21, sc.HAND21_KPTS, sc.HAND21_PAFS
    if name == "guide5":
        return 5, sc.GUIDE5_KPTS, sc.GUIDE5_PAFS
    raise KeyError(name)


def train_limbs(limb_kpts, limb_pafs):
    """The table in coco.py's order: row j is the limb whose PAF channels are (2j, 2j + 1)."""
    out = [None] * len(limb_kpts)
    for (a, b), (c0, c1) in zip(limb_kpts, limb_pafs):
        assert c0 % 2 == 0 and c1 == c0 + 1 and out[c0 // 2] is None, (c0, c1)
        out[c0 // 2] = [int(a), int(b)]
    return out


def _canon(name):
    if name == "coco":
        return _CANON18
    c = np.array(sc.HAND21_CANON if name == "hand21" else sc.GUIDE5_CANON, dtype=np.float64)
    c = c - c.min(0)
    return c / c.max()


def _person(rng, name, H, W, spread=1.0, p_vis2=0.15):
    """A canonical figure somewhere in (and a little around) the frame, jittered; visibility 0 / 1, some 2."""
    c = _canon(name)
    size = np.array([W, H]) * rng.uniform(0.5, 1.1) * spread
    org = np.array([rng.uniform(-0.15 * W, 0.6 * W), rng.uniform(-0.15 * H, 0.6 * H)])
    xy = org + c * size + rng.uniform(-1.5, 1.5, size=c.shape)
    vis = rng.randint(0, 2, size=len(c)).astype(np.float64)
    vis[rng.rand(len(c)) < p_vis2] = 2.0
    return np.concatenate([xy, vis[:, None]], 1)


def _blank(K):
    p = np.zeros((K, 3))
    p[:, 2] = 2.0
    return p


def _borders(rng):
    a = _person(rng, "coco", 48, 40)
    a[0] = (20.3, 11.9, 0)                               # inside the frame
    b = _blank(18)
    b[0] = (3.5, 3.5, 1)                                 # exactly on a cell centre: exponent 0, increment 1
    b[1] = (-5.0, -3.0, 0)                               # negative coordinates, within reach
    b[2] = (47.0, 54.0, 1)                               # beyond the far corner, within reach
    b[3] = (40.0, 20.0, 0)                               # x == W exactly
    b[4] = (-40.0, 10.0, 0)                              # out of reach: br < tl, nothing touched
    b[5] = (17.0, 23.0, 2)                               # visibility 2 does not count
    b[6] = (17.0, 23.0, 1)                               # visibility 1 does
    b[7] = (39.999, 47.999, 0)
    c = a.copy()                                         # a second person on the same spots: the clip to 1 fires
    c[:, 2] = np.minimum(c[:, 2], 1.0)
    return [[a, b, c], [], [_person(rng, "coco", 48, 40)]]


def _paf_specials(rng):
    p = _blank(18)
    p[1] = (12.0, 16.0, 0); p[2] = (28.0, 16.0, 0)       # limb [1,2] along y = 2.0 map units: row 1 lies at d == thickness 1
    p[8] = (12.0, 16.0, 1)                               # limb [1,8]: zero length
    p[5] = (30.0, 30.0, 2)                               # limb [1,5]: one end with visibility 2
    p[11] = (-20.0, 60.0, 0)                             # limb [1,11]: partly outside the frame
    p[9] = (20.0, 44.0, 0)                               # limb [8,9]: vertical, x = 1.5 map units
    q = _blank(18)
    q[5] = (36.0, 8.0, 0); q[6] = (70.0, 40.0, 1)        # limb [5,6] leaves the frame on the right
    q[14] = (10.0, 4.0, 0); q[16] = (30.0, 44.0, 0)      # limb [14,16], oblique
    return [[p, q]]


def _cross(order):
    p, q = _blank(18), _blank(18)
    p[1] = (4.0, 4.0, 0); p[2] = (36.0, 44.0, 0)         # limb [1,2] of two persons crossing near the middle of the frame
    q[1] = (36.0, 4.0, 0); q[2] = (4.0, 44.0, 1)
    return [[p, q] if order == 0 else [q, p]]


def _crowd(rng, name, H, W, counts):
    return [[_person(rng, name, H, W, spread=0.6) for _ in range(n)] for n in counts]


# name -> (skeleton, H, W, stride, sigma, paf_thickness, frames); a frame is its persons in label order, (K, 3) each
def build_cases():
    rng = np.random.RandomState(20260)
    cases = {}
    cases["borders"] = ("coco", 48, 40, 8, 7, 1, _borders(rng))
    cases["odd_45x43"] = ("coco", 45, 43, 8, 7, 1, _crowd(rng, "coco", 45, 43, [2, 3]))
    cases["stride4_sigma3p5"] = ("coco", 48, 40, 4, 3.5, 2, _crowd(rng, "coco", 48, 40, [3]))
    cases["chunk"] = ("coco", 48, 40, 8, 7, 1, _crowd(rng, "coco", 48, 40, [CHUNK - 1, CHUNK, CHUNK + 1]))
    cases["two_chunks_plus"] = ("coco", 48, 40, 8, 7, 1, _crowd(rng, "coco", 48, 40, [2 * CHUNK + 3]))
    cases["paf_t1"] = ("coco", 48, 40, 8, 7, 1, _paf_specials(rng))
    cases["paf_t2"] = ("coco", 48, 40, 8, 7, 2, _paf_specials(rng))
    cases["cross_ab"] = ("coco", 48, 40, 8, 7, 1, _cross(0))
    cases["cross_ba"] = ("coco", 48, 40, 8, 7, 1, _cross(1))
    cases["hand21"] = ("hand21", 48, 40, 8, 7, 1, _crowd(rng, "hand21", 48, 40, [2, 0, CHUNK + 1]))
    cases["hand21_stride4"] = ("hand21", 45, 43, 4, 3.5, 2, _crowd(rng, "hand21", 45, 43, [3]))
    cases["guide5"] = ("guide5", 48, 40, 8, 7, 1, _crowd(rng, "guide5", 48, 40, [3, 1]))
    return cases


COCO_CASES = ["borders", "odd_45x43", "stride4_sigma3p5", "chunk", "two_chunks_plus", "paf_t1", "paf_t2", "cross_ab", "cross_ba"]
CUSTOM_CASES = ["hand21", "hand21_stride4", "guide5"]


def frames_to_arrays(frames, K):
    """(kpts (N, Pmax, K, 3) float64, n_persons (N,) int32); unused rows hold visibility 2."""
    n = np.array([len(f) for f in frames], np.int32)
    kpts = np.zeros((len(frames), int(n.max()), K, 3))
    kpts[..., 2] = 2.0
    for f, persons in enumerate(frames):
        for i, p in enumerate(persons):
            kpts[f, i] = p
    return kpts, n


def frames_to_labels(frames, K):
    """The same persons as label dicts of prepare_train_labels.py's format.  The format always has a main person: a frame
    without persons becomes a main person whose key-points all have visibility 2."""
    labels = []
    for persons in frames:
        persons = persons if persons else [_blank(K)]
        labels.append({"keypoints": persons[0].tolist(),
                       "processed_other_annotations": [{"keypoints": p.tolist()} for p in persons[1:]]})
    return labels


# ------------------------------------------------------------------------------------------------ restatement, vectorised
def targets(kpts, n_persons, H, W, stride, sigma, thickness, K, limbs):
    """keypoint_maps (N, K + 1, h, w), paf_maps (N, 2L, h, w) float32; ``limbs``: rows (a, b, channel x, channel y)."""
    N, h, w = len(n_persons), H // stride, W // stride
    L = len(limbs)
    kmaps = np.zeros((N, K + 1, h, w), np.float32)
    pmaps = np.zeros((N, 2 * L, h, w), np.float32)
    shift = stride / 2 - 0.5
    gx, gy = np.arange(w), np.arange(h)
    for f in range(N):
        P = int(n_persons[f])
        for k in range(K):
            m = kmaps[f, k]
            for q in range(P):
                x, y, v = (float(t) for t in kpts[f, q, k])
                if not v <= 1:
                    continue
                tl = [max(int(x - 4 * sigma), 0), max(int(y - 4 * sigma), 0)]
                br = [min(int(x + 4 * sigma), w * stride), min(int(y + 4 * sigma), h * stride)]
                inx = (gx >= tl[0] // stride) & (gx < br[0] // stride)
                iny = (gy >= tl[1] // stride) & (gy < br[1] // stride)
                ax, ay = gx * stride + shift - x, gy * stride + shift - y
                e = ((ax * ax)[None, :] + (ay * ay)[:, None]) / 2 / sigma / sigma
                sel = inx[None, :] & iny[:, None] & ~(e > 4.6052)
                m[sel] = np.minimum(m[sel] + np.exp(-e[sel]).astype(np.float32), np.float32(1))
        kmaps[f, K] = 1 - kmaps[f].max(axis=0)
        for a, b, c0, c1 in limbs:
            for q in range(P):
                xa, ya, va = (float(t) for t in kpts[f, q, a])
                xb, yb, vb = (float(t) for t in kpts[f, q, b])
                if not (va <= 1 and vb <= 1):
                    continue
                xa /= stride; ya /= stride; xb /= stride; yb /= stride
                xba, yba = xb - xa, yb - ya
                x0, x1 = int(max(min(xa, xb) - thickness, 0)), int(min(max(xa, xb) + thickness, w))
                y0, y1 = int(max(min(ya, yb) - thickness, 0)), int(min(max(ya, yb) + thickness, h))
                norm = (xba * xba + yba * yba) ** 0.5
                if norm < 1e-7:
                    continue
                xba /= norm; yba /= norm
                d = np.abs((gx - xa)[None, :] * yba - (gy - ya)[:, None] * xba)
                sel = (d <= thickness) & ((gx >= x0) & (gx < x1))[None, :] & ((gy >= y0) & (gy < y1))[:, None]
                pmaps[f, c0][sel] = xba
                pmaps[f, c1][sel] = yba
    return kmaps, pmaps


def limb_rows(limb_kpts, limb_pafs):
    return [(int(a), int(b), int(c0), int(c1)) for (a, b), (c0, c1) in zip(limb_kpts, limb_pafs)]


def targets_loops(kpts, n_persons, H, W, stride, sigma, thickness, K, limbs):
    """The same targets with one Python iteration per touched pixel, the way the reference's dataset renders them."""
    N, h, w = len(n_persons), H // stride, W // stride
    kmaps = np.zeros((N, K + 1, h, w), np.float32)
    pmaps = np.zeros((N, 2 * len(limbs), h, w), np.float32)
    shift = stride / 2 - 0.5
    for f in range(N):
        P = int(n_persons[f])
        for k in range(K):
            m = kmaps[f, k]
            for q in range(P):
                x, y, v = (float(t) for t in kpts[f, q, k])
                if not v <= 1:
                    continue
                x0, y0 = max(int(x - 4 * sigma), 0) // stride, max(int(y - 4 * sigma), 0) // stride
                x1, y1 = min(int(x + 4 * sigma), w * stride) // stride, min(int(y + 4 * sigma), h * stride) // stride
                for my in range(y0, y1):
                    for mx in range(x0, x1):
                        ax, ay = mx * stride + shift - x, my * stride + shift - y
                        e = (ax * ax + ay * ay) / 2 / sigma / sigma
                        if e > 4.6052:
                            continue
                        m[my, mx] += math.exp(-e)
                        if m[my, mx] > 1:
                            m[my, mx] = 1
        kmaps[f, K] = 1 - kmaps[f].max(axis=0)
        for a, b, c0, c1 in limbs:
            for q in range(P):
                xa, ya, va = (float(t) for t in kpts[f, q, a])
                xb, yb, vb = (float(t) for t in kpts[f, q, b])
                if not (va <= 1 and vb <= 1):
                    continue
                xa /= stride; ya /= stride; xb /= stride; yb /= stride
                xba, yba = xb - xa, yb - ya
                norm = (xba * xba + yba * yba) ** 0.5
                if norm < 1e-7:
                    continue
                xba /= norm; yba /= norm
                for my in range(int(max(min(ya, yb) - thickness, 0)), int(min(max(ya, yb) + thickness, h))):
                    for mx in range(int(max(min(xa, xb) - thickness, 0)), int(min(max(xa, xb) + thickness, w))):
                        if math.fabs((mx - xa) * yba - (my - ya) * xba) <= thickness:
                            pmaps[f, c0, my, mx] = xba
                            pmaps[f, c1, my, mx] = yba
    return kmaps, pmaps


def mask_mean(mask, stride):
    """(N, H, W) -> (N, H / stride, W / stride): block means in float64, rounded once (exact for 0 / 1 masks)."""
    N, H, W = mask.shape
    assert H % stride == 0 and W % stride == 0
    return mask.astype(np.float64).reshape(N, H // stride, stride, W // stride, stride).mean(axis=(2, 4)).astype(np.float32)


def l2_loss64(out, target, mask, batch_size):
    """modules/loss.py in float64 on float32 inputs; mask (N, h, w) broadcast over the channels."""
    d = (out.astype(np.float64) - target.astype(np.float64)) * mask.astype(np.float64)[:, None]
    return float((d * d / 2 / batch_size).sum())


# ------------------------------------------------------------------------------------------------ comparisons
def ulp_distance(a, b):
    """Per element, how many float32 steps apart (0 = identical bits up to the sign of zero)."""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def touched(m):
    return m != 0


# ------------------------------------------------------------------------------------------------ loss cases
# name -> (N, heat-map channels, PAF channels, h, w, seed): synthetic stage tensors, targets and a mask with zeros
LOSS_CASES = {"small": (2, 19, 38, 6, 5, 1), "multi_block": (3, 19, 38, 46, 46, 2), "guide5": (2, 6, 8, 6, 5, 3)}


def loss_inputs(name, n_stages=2):
    N, CH, CP, h, w, seed = LOSS_CASES[name]
    rng = np.random.RandomState(1000 + seed)
    kt = rng.rand(N, CH, h, w).astype(np.float32)
    pt = (rng.rand(N, CP, h, w).astype(np.float32) * 2 - 1) * (rng.rand(N, CP, h, w) < 0.2)
    mask = (rng.rand(N, h, w) > 0.25).astype(np.float32)
    mask[0, 0, :2] = 0.5                                 # a block the mask's down-sampling averaged
    outs = []
    for s in range(n_stages):
        outs.append((kt + rng.randn(N, CH, h, w) * 0.1).astype(np.float32))
        outs.append((pt + rng.randn(N, CP, h, w) * 0.1).astype(np.float32))
    return outs, kt, pt.astype(np.float32), mask
