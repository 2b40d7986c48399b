"""Custom-skeleton grouping cases (plain data + deterministic builders), shared by tools/make_skeleton_golden.py and the
tests that replay tests/golden/skeleton_*.npz.  Maps and key-point lists are regenerated from these definitions; the
fixtures hold parameters, input digests and the reference's outputs only."""
import hashlib

import numpy as np

from lwpose_amd import synth

# guide5: TRAIN-ON-CUSTOM-DATASET.md's example (num_heatmaps = 6, num_pafs = 8), a rooted tree: neck, hip, two feet, head
GUIDE5_CANON = [[0.0, 0.0], [0.0, 0.9], [-0.25, 1.9], [0.25, 1.9], [0.0, -0.4]]
GUIDE5_KPTS = [[0, 1], [1, 2], [1, 3], [0, 4]]
GUIDE5_PAFS = [[0, 1], [2, 3], [4, 5], [6, 7]]

# hand21: wrist + five fingers of four joints; the 20 limbs go wrist -> finger base -> ... -> tip, so limbs 17 and 18 (the
# reference's fill-a-missing-end rule, keypoints.py:166-175) are the middle bones of the little finger, not closing limbs
HAND21_CANON = [[0.0, 2.0]] + [[-0.8 + 0.4 * f, 1.35 - 0.42 * j] for f in range(5) for j in range(4)]
HAND21_KPTS = [[0 if j == 0 else 1 + 4 * f + j - 1, 1 + 4 * f + j] for f in range(5) for j in range(4)]
HAND21_PAFS = [[2 * ((7 * l + 3) % 20), 2 * ((7 * l + 3) % 20) + 1] for l in range(20)]    # permuted channel pairs

# coco_dense: the COCO tables plus neck -> every type that no COCO limb joins to the neck (PAF channels 38 ..)
COCO_KPTS = [list(p) for p in synth.LIMB_KPTS]
COCO_PAFS = [list(p) for p in synth.LIMB_PAFS]
_NECK_EXTRA = [t for t in range(18) if t != 1 and [1, t] not in COCO_KPTS]
DENSE_KPTS = COCO_KPTS + [[1, t] for t in _NECK_EXTRA]
DENSE_PAFS = COCO_PAFS + [[38 + 2 * i, 39 + 2 * i] for i in range(len(_NECK_EXTRA))]
COCO_CANON = synth._CANON.tolist()

# (name, canon, limb_kpts, limb_pafs, num_pafs, n_people, h, w, seed, drop_prob, noise, ratio)
MAP_CASES = [
    ("guide5_r4", GUIDE5_CANON, GUIDE5_KPTS, GUIDE5_PAFS, 8, 4, 40, 64, 11, 0.05, 0.01, 4),
    ("guide5_r8", GUIDE5_CANON, GUIDE5_KPTS, GUIDE5_PAFS, 8, 3, 24, 40, 12, 0.05, 0.01, 8),
    ("hand21", HAND21_CANON, HAND21_KPTS, HAND21_PAFS, 40, 3, 64, 96, 13, 0.0, 0.005, 4),
    ("coco_dense", COCO_CANON, DENSE_KPTS, DENSE_PAFS, 2 * len(DENSE_KPTS), 4, 46, 82, 14, 0.1, 0.01, 4),
]

# coco_options: the default tables on existing post_p*.npz maps (oracle/make_golden.py POST_CASES), other options.  The PAF
# field of limb l is scaled by OPTION_PAF_SCALE[l % 3] so that line-integral samples fall on both sides of 0.05 and of 0.2:
# scale 0.1 passes 0.05 but not 0.2, scale 0.03 passes 0.0 but not 0.05 (the raw fields sit near 1 or near 0 +- noise, where
# every threshold in 0.0 .. 0.2 decides alike).
# (name, post case params (n_people, h, w, seed, drop_prob, noise, ratio), pose_entry_size, min_paf_score)
OPTION_PAF_SCALE = (1.0, 0.1, 0.03)
OPTION_CASES = [
    ("coco_options_p5_s00", (5, 46, 82, 4, 0.15, 0.02, 4), 24, 0.0),
    ("coco_options_p5_s02", (5, 46, 82, 4, 0.15, 0.02, 4), 24, 0.2),
    ("coco_options_r8_s00", (2, 16, 24, 7, 0.0, 0.01, 8), 24, 0.0),
    ("coco_options_r8_s02", (2, 16, 24, 7, 0.0, 0.01, 8), 24, 0.2),
]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def map_case(name):
    for c in MAP_CASES:
        if c[0] == name:
            return c
    raise KeyError(name)


def make_maps(case):
    """Low-resolution (heat (K+1,h,w), paf (num_pafs,h,w)) of a MAP_CASES row."""
    _, canon, kpts, pafs, npafs, n, h, w, seed, drop, noise, _ = case
    heat, paf, _ = synth.make_skeleton_maps(canon, kpts, pafs, npafs, n, h, w, seed, drop, noise)
    return heat, paf


def option_maps(params):
    """Low-resolution maps of an OPTION_CASES row: make_pose_maps, then limb l's two PAF channels times OPTION_PAF_SCALE[l % 3]."""
    n, h, w, seed, drop, noise, _ = params
    heat, paf, _ = synth.make_pose_maps(n, h, w, seed, drop, noise)
    for l, (c0, c1) in enumerate(COCO_PAFS):
        for c in (c0, c1):
            paf[c] = (paf[c] * np.float32(OPTION_PAF_SCALE[l % 3])).astype(np.float32)
    return heat, paf


def _kp(x, y, s, i):
    return (np.int64(x), np.int64(y), np.float32(s), i)


def adversarial_cases():
    """Hand-made key-point lists (as oracle/make_golden.py gen_group_adversarial does for COCO):
    name -> (K, limb_kpts, limb_pafs, by_type lists, pafs (H,W,C) float32)."""
    out = {}
    H, W = 64, 96
    # a type that no limb uses (type 5 has key-points, no limb names it)
    paf = np.zeros((H, W, 8), np.float32); paf[:, :, 1] = 1.0; paf[:, :, 3] = 1.0; paf[:, :, 5] = 1.0
    bt = [[_kp(x + p, y, 0.6 + 0.05 * t, 2 * t + p) for p, x in enumerate((20, 60))] for t, y in enumerate((10, 24, 38, 52))]
    bt += [[], [_kp(40, 30, 0.9, 8), _kp(80, 30, 0.8, 9)]]           # ids: the running index in type order
    out["unused_type"] = (6, [[0, 1], [1, 2], [2, 3]], [[0, 1], [2, 3], [4, 5]], bt, paf)
    # a limb listed twice (every connection is applied twice: counts and scores grow twice)
    out["limb_twice"] = (6, [[0, 1], [1, 2], [1, 2], [2, 3]], [[0, 1], [2, 3], [2, 3], [4, 5]],
                         [list(l) for l in bt], paf)
    # a zero-length pair: types 0 and 1 at the same pixel (skipped, keypoints.py:106-107), plus a regular person
    paf = np.zeros((H, W, 6), np.float32); paf[:, :, 1] = 1.0; paf[:, :, 3] = 1.0; paf[:, :, 5] = 1.0
    bt = [[_kp(30, 20, 0.9, 0), _kp(70, 10, 0.8, 1)], [_kp(30, 20, 0.7, 2), _kp(70, 24, 0.7, 3)],
          [_kp(30, 34, 0.6, 4), _kp(70, 38, 0.6, 5)], [_kp(70, 52, 0.5, 6)]]
    out["zero_length"] = (4, [[0, 1], [1, 2], [2, 3]], [[0, 1], [2, 3], [4, 5]], bt, paf)
    # a one-sided limb at index 0 (type 0 has no key-points: limb 0 seeds single-key-point entries, no part_id == 0 reset)
    bt = [[], [_kp(30, 20, 0.7, 0), _kp(70, 24, 0.7, 1)], [_kp(30, 34, 0.6, 2), _kp(70, 38, 0.6, 3)], [_kp(70, 52, 0.5, 4)]]
    out["one_sided_first"] = (4, [[0, 1], [1, 2], [2, 3]], [[0, 1], [2, 3], [4, 5]], bt, paf)
    # more than 64 candidates on one limb: 9 x 9 pairs under a uniform field pass the line integral (81 candidates)
    H2, W2 = 128, 96
    paf = np.zeros((H2, W2, 4), np.float32); paf[:, :, 0] = 1.0; paf[:, :, 2] = 1.0
    bt = [[_kp(10, 10 + 5 * i, 0.5 + 0.01 * i, i) for i in range(9)], [_kp(50, 12 + 5 * j, 0.6 + 0.01 * j, 9 + j) for j in range(9)],
          [_kp(90, 10 + 5 * j, 0.7, 18 + j) for j in range(9)]]
    out["many_candidates"] = (3, [[0, 1], [1, 2]], [[0, 1], [2, 3]], bt, paf)
    # more than 64 entries that survive the filter: 70 vertical three-key-point people, each limb's field only on its own
    # column (70 candidates per limb, all picked), so entries 64.. spill past the LDS rows of the generic assembly
    H3, W3, P = 64, 300, 70
    paf = np.zeros((H3, W3, 4), np.float32)
    bt = [[], [], []]
    for p in range(P):
        x = 5 + 4 * p
        paf[:, x, 1] = 1.0; paf[:, x, 3] = 1.0
        for t, y in enumerate((10, 22, 34)):
            bt[t].append(_kp(x, y, 0.5 + 0.004 * p, t * P + p))
    out["spill"] = (3, [[0, 1], [1, 2]], [[0, 1], [2, 3]], bt, paf)
    return out


def flat_kp(by_type):
    """(n,5) rows x, y, score, id, type of a by-type key-point list."""
    return np.array([[p[0], p[1], p[2], p[3], t] for t, l in enumerate(by_type) for p in l], dtype=np.float64).reshape(-1, 5)


def by_type_from_flat(kp, K):
    bt = [[] for _ in range(K)]
    for x, y, s, i, t in kp:
        bt[int(t)].append((np.int64(x), np.int64(y), np.float32(s), int(i)))
    return bt
