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
    if name in ("chain33", "chain64"):                   # synthetic: limb j joins types (j, j + 1) and owns PAF channels (2j, 2j + 1)
        K = int(name[5:])
        return K, [[j, j + 1] for j in range(K - 1)], [[2 * j, 2 * j + 1] for j in range(K - 1)]
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


# ------------------------------------------------------------------------------------------------ cases past one workgroup
# The cases above never leave the targets kernel's smallest form: at most 120 map pixels (one workgroup of 256 threads), at
# most 8 x 21 = 168 staged chunk entries (one trip of the 256-thread staging loop).  The ones below do; what each is for is
# asserted by tools/make_train_golden.py and again, on the fixture, by tests/test_train_host.py.
def _row257(rng):
    a = _blank(18)
    a[0] = (2046.0, 4.0, 0)                              # between the centres of pixels 255 (x = 2043.5) and 256 (2051.5)
    a[1] = (2030.0, 4.0, 0); a[2] = (2054.0, 4.0, 1)     # limb [1,2]: 253.75 .. 256.75 map units, across the 255 / 256 boundary
    a[3] = (2056.0, 3.5, 0)                              # x == W exactly
    a[4] = (2051.5, 3.5, 1)                              # the centre of pixel 256, the last one: increment 1
    a[5] = (2043.5, 3.5, 0)                              # the centre of pixel 255, the first workgroup's last thread
    b = _blank(18)
    b[:, 0] = rng.uniform(2000.0, 2070.0, 18)            # around the far end and up to 14 px beyond it
    b[:, 1] = rng.uniform(-10.0, 18.0, 18)
    b[:, 2] = rng.randint(0, 3, 18)
    return [[a, b, _person(rng, "coco", 8, 2056)]]


def _grid272(rng):
    frames = _crowd(rng, "coco", 136, 128, [3, CHUNK + 2, 0])
    frames[1][0][0] = (60.0, 130.0, 0)                   # persons 0 and 9 of frame 1, chunks 0 and 1, on one cell of the last map row
    frames[1][CHUNK + 1][0] = (62.0, 128.0, 1)           # (pixel 16 * 16 + 7 = 263 of workgroup 1): 0.975 + 0.828, clipped to 1
    return frames


def _interior(rng):
    a = _blank(18)
    a[0] = (60.0, 90.0, 0)                               # x - 4 sigma == 32.0, a multiple of the stride: the box starts at cell 4
    a[1] = (100.0, 64.0, 0); a[2] = (140.0, 64.0, 0)     # limb [1,2] along y = 8.0 map units: row 7 lies at d == thickness 1
    a[5] = (40.0, 40.0, 0); a[6] = (90.0, 110.0, 1)      # limb [5,6], oblique
    a[8] = (100.0, 100.0, 0); a[9] = (103.0, 101.0, 0)   # limb [8,9], 0.4 map units long
    a[11] = (150.0, 40.0, 1); a[12] = (150.0, 120.0, 0)  # limb [11,12], vertical at x = 18.75 map units
    b = _blank(18)
    b[0] = (59.9, 130.0, 1)                              # a hair below: int(31.9) = 31, the box starts at cell 3
    b[3] = (172.0, 156.0, 0)                             # x + 4 sigma == W, y + 4 sigma == H: the far clamps change nothing
    b[4] = (28.0, 28.0, 0)                               # x - 4 sigma == 0, y - 4 sigma == 0
    c = a.copy()                                         # a second person on the same spots: the clip to 1 fires mid-map
    c[:, 2] = np.minimum(c[:, 2], 1.0)
    return [[a, b, c], _crowd(rng, "coco", 184, 200, [2])[0]]          # frame 0 is hand-placed only, frame 1 two figures


def _stride4_grid(rng):
    frames = _crowd(rng, "coco", 72, 64, [3])
    p = _blank(18)
    p[0] = (30.0, 68.0, 0)                               # map row 17, pixels 272 and above
    p[1] = (10.0, 66.0, 0); p[2] = (50.0, 70.0, 1)       # limb [1,2] across rows 16 and 17
    frames[0].append(p)
    return frames


def _scatter(rng, K, H, W, counts):
    """Key-points uniform over the frame and 20 px beyond it, visibility 0 / 1 / 2 in equal parts."""
    def one():
        p = np.zeros((K, 3))
        p[:, 0] = rng.uniform(-20.0, W + 20.0, K)
        p[:, 1] = rng.uniform(-20.0, H + 20.0, K)
        p[:, 2] = rng.randint(0, 3, K)
        return p
    return [[one() for _ in range(n)] for n in counts]


def _chain33(rng):
    frames = _scatter(rng, 33, 136, 128, [CHUNK + 3])
    frames[0][CHUNK - 1][25:, 2] = [0, 1, 0, 1, 2, 0, 1, 0]   # person 7, types 25 .. 32: chunk entries 256 .. 263, the second staging trip
    return frames


def build_grid_cases():
    rng = np.random.RandomState(20261)
    cases = {}
    cases["row257"] = ("coco", 8, 2056, 8, 7, 1, _row257(rng))                 # 1 x 257: the second workgroup has one active thread
    cases["full256"] = ("coco", 128, 128, 8, 7, 1, _crowd(rng, "coco", 128, 128, [3]))   # 16 x 16: one workgroup, no inactive thread
    cases["grid272"] = ("coco", 136, 128, 8, 7, 1, _grid272(rng))              # 17 x 16, frames of 3 / CHUNK + 2 / 0 persons
    cases["interior"] = ("coco", 184, 200, 8, 7, 1, _interior(rng))            # 23 x 25 = 575 pixels, three workgroups
    cases["stride4_grid"] = ("coco", 72, 64, 4, 3.5, 2, _stride4_grid(rng))    # 18 x 16 = 288
    cases["chain33"] = ("chain33", 136, 128, 8, 7, 1, _chain33(rng))           # 8 x 33 = 264 chunk entries
    cases["chain64"] = ("chain64", 136, 128, 8, 7, 1, _scatter(rng, 64, 136, 128, [CHUNK, CHUNK + 3]))   # 512 entries, 20 KB of LDS
    return cases


GRID_CASES = ["row257", "full256", "grid272", "interior", "stride4_grid", "chain33", "chain64"]
GRID_PIXELS = {"row257": 257, "full256": 256, "grid272": 272, "interior": 575, "stride4_grid": 288, "chain33": 272, "chain64": 272}
PAST_256 = ["row257", "grid272", "interior", "stride4_grid"]      # coco cases that touch pixels of linear index 256 or above
TARGET_FILES = {"train_targets": COCO_CASES, "train_targets_custom": CUSTOM_CASES, "train_targets_grid": GRID_CASES}


def all_cases():
    cases = build_cases()
    cases.update(build_grid_cases())
    return cases


def gaussian_box(x, y, sigma, stride, h, w):
    """_add_gaussian's cell range (x0, x1, y0, y1) and whether each of its four edges was clamped by the frame."""
    tl = [int(x - 4 * sigma), int(y - 4 * sigma)]
    br = [int(x + 4 * sigma), int(y + 4 * sigma)]
    clamped = (tl[0] < 0, br[0] > w * stride, tl[1] < 0, br[1] > h * stride)
    return (max(tl[0], 0) // stride, min(br[0], w * stride) // stride, max(tl[1], 0) // stride, min(br[1], h * stride) // stride), clamped


def check_grid_cases(cases, maps):
    """What every grid case is for, asserted on ``maps``: name -> (keypoint_maps, paf_maps) as the reference rendered them."""
    for name in GRID_CASES:
        skel, H, W, stride, sigma, thick, frames = cases[name]
        k, p = maps[name]
        assert k.shape[2] * k.shape[3] == GRID_PIXELS[name] == (H // stride) * (W // stride), name
        K = skeleton(skel)[0]
        flat_k, flat_p = k[:, :K].reshape(len(frames), K, -1), p.reshape(len(frames), p.shape[1], -1)
        if name in PAST_256:
            assert flat_k[..., 256:].any() and flat_p[..., 256:].any(), name
    k, p = maps["row257"]
    assert k.shape[2:] == (1, 257) and k[0, 0, 0, 255] != 0 and k[0, 0, 0, 256] != 0 and k[0, 4, 0, 256] == 1.0 and k[0, 5, 0, 255] == 1.0
    assert (p[0, 12, 0, 252:257] != 0).all()                                           # limb [1,2] on both sides of the boundary
    k, p = maps["grid272"]
    assert [len(f) for f in cases["grid272"][6]] == [3, CHUNK + 2, 0]
    assert k[1, 0, 16, 7] == 1.0 and not k[2, :18].any() and (k[2, 18] == 1).all() and not p[2].any()
    skel, H, W, stride, sigma, thick, frames = cases["interior"]
    k, p = maps["interior"]
    h, w = H // stride, W // stride
    boxes = [gaussian_box(x, y, sigma, stride, h, w) for person in frames[0] for x, y, v in person if v <= 1]
    assert any(not any(c) and 0 < b[0] and b[1] < w and 0 < b[2] and b[3] < h for b, c in boxes)   # four unclamped edges inside the map
    on, below = gaussian_box(*frames[0][0][0][:2], sigma, stride, h, w)[0], gaussian_box(*frames[0][1][0][:2], sigma, stride, h, w)[0]
    assert frames[0][0][0][0] - 4 * sigma == 32.0 and on[0] == 4 and below[0] == 3      # the boundary pair lands in different cells
    assert k[0, 0, 11, 7] == 1.0 and (k[0, :18, 2:-2, 2:-2] == 1.0).sum() > 3           # the clip fired away from every border
    assert p[0, 12, 7, 14] == 1.0 and p[0, 12, 8, 14] == 1.0 and p[0, 12, 6, 14] == 0.0 and p[0, 12, 9, 14] == 0.0   # row 7: d == thickness
    for c in (2, 22, 8):                                                                # short, oblique and vertical limbs, wholly inside
        assert p[0, c:c + 2].any() and not p[0, c:c + 2, 0].any() and not p[0, c:c + 2, -1].any()
        assert not p[0, c:c + 2, :, 0].any() and not p[0, c:c + 2, :, -1].any()
    skel, H, W, stride, sigma, thick, frames = cases["chain33"]
    assert len(frames[0]) == CHUNK + 3
    late = [(x, y) for x, y, v in frames[0][CHUNK - 1][25:] if v <= 1]                  # chunk entries 7 * 33 + 25 = 256 and above
    assert late and any(b[0] < b[1] and b[2] < b[3] for b in (gaussian_box(x, y, sigma, stride, H // stride, W // stride)[0] for x, y in late))
    assert sorted(len(f) for f in cases["chain64"][6]) == [CHUNK, CHUNK + 3] and skeleton("chain64")[0] == 64


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


# ------------------------------------------------------------------------------------------------ mask cases
# (N, H, W, stride): 272 cells in two workgroups with frame offsets; 1 x 257; an odd stride on 17 x 16; stride 1 (a copy, 300
# cells); 256-cell blocks on a 4 x 3 map
MASK_CASES = [(2, 136, 128, 8), (1, 8, 2056, 8), (3, 51, 48, 3), (1, 20, 15, 1), (2, 64, 48, 16)]


def mask_input(case, kind):
    """``binary``: 0 / 1.  ``fraction``: multiples of 2^-8 in [0, 1], so that a block of at most 256 cells sums exactly in double
    (the sum times 256 is an integer below 2^17) and the one correct rounding of the mean is the only answer."""
    N, H, W, stride = case
    rng = np.random.RandomState(100 * H + W + stride)
    if kind == "binary":
        return (rng.rand(N, H, W) > 0.4).astype(np.float32)
    assert kind == "fraction"
    return (rng.randint(0, 257, size=(N, H, W)) / 256.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ loss cases
# name -> (N, heat-map channels, PAF channels, h, w, seed): synthetic stage tensors, targets and a mask with zeros
LOSS_CASES = {"small": (2, 19, 38, 6, 5, 1), "multi_block": (3, 19, 38, 46, 46, 2), "guide5": (2, 6, 8, 6, 5, 3)}
# past the loss grid's cap of 1024 workgroups x 256 positions = 262 144, and past 16 tensors (guide5 channels throughout)
LOSS_CAP = 1024 * 256
LOSS_GRID_CASES = {"cap_exact": (1, 6, 8, 512, 512, 11),         # 262 144 positions: 1024 workgroups, one trip
                   "one_past_cap": (5, 6, 8, 1, 52429, 12),      # 262 145: the second trip is one position, and it carries the loss
                   "second_trip": (2, 6, 8, 363, 363, 13),       # 263 538
                   "s18": (2, 6, 8, 6, 5, 14),                   # 18 tensors (8 refinement stages): two launches
                   "s18_46": (2, 6, 8, 46, 46, 15)}              # ... whose partials fill more than one workgroup
LOSS_GRID_STAGES = {"cap_exact": 1, "one_past_cap": 1, "second_trip": 1, "s18": 9, "s18_46": 9}


def loss_inputs(name, n_stages=2):
    N, CH, CP, h, w, seed = LOSS_CASES[name] if name in LOSS_CASES else LOSS_GRID_CASES[name]
    rng = np.random.RandomState(1000 + seed)
    kt = rng.rand(N, CH, h, w).astype(np.float32)
    pt = (rng.rand(N, CP, h, w).astype(np.float32) * 2 - 1) * (rng.rand(N, CP, h, w) < 0.2)
    mask = (rng.rand(N, h, w) > 0.25).astype(np.float32)
    mask[0, 0, :2] = 0.5                                 # a block the mask's down-sampling averaged
    outs = []
    for s in range(n_stages):
        outs.append((kt + rng.randn(N, CH, h, w) * 0.1).astype(np.float32))
        outs.append((pt + rng.randn(N, CP, h, w) * 0.1).astype(np.float32))
    pt = pt.astype(np.float32)
    if name == "one_past_cap":                           # the very last position: an error of 1 in every channel, mask 1
        mask[-1, -1, -1] = 1.0
        for i, o in enumerate(outs):
            o[-1, :, -1, -1] = (pt if i % 2 else kt)[-1, :, -1, -1] + np.float32(1)
    return outs, kt, pt, mask


def l2_loss64_first(out, target, mask, batch_size, positions):
    """A wrong l2_loss64: the sum over the first ``positions`` (frame, pixel) positions only."""
    N, C, h, w = out.shape
    keep = (np.arange(N * h * w) < positions).reshape(N, 1, h, w)
    d = (out.astype(np.float64) - target.astype(np.float64)) * mask.astype(np.float64)[:, None]
    return float((d * d / 2 / batch_size * keep).sum())
