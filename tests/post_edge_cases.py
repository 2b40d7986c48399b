"""Edge cases of the post-processing chain (plain data + deterministic builders), shared by tools/make_post_edge_golden.py and
the tests that replay tests/golden/post_edge_*.npz.  Every case is built to land on a count where a kernel of
csrc/post_kernels.hip switches form ("boundary table"); its ``expect`` dict states that count, and
``check_expect`` verifies it against the oracle's counts on the CPU.  Inputs are rebuilt from these definitions; the fixtures
hold input digests and the reference's outputs only.

Three kinds of case:
  "group"  hand-placed by-type key-point lists + a full-resolution PAF (H,W,38)        -> Engine.group_keypoints / the drop-in
  "full"   a full-resolution heat map (H,W,19) of single-pixel spikes + a zero PAF     -> poses_from_maps(ratio 1, NHWC) and the
           drop-in extract_keypoints per channel (find_peaks_kernel<1,..> + nms_kernel)
  "maps"   low-resolution heat (19,h,w) / PAF (38,h,w)                                 -> poses_from_maps(ratio 4 / 8, NCHW)

Facts the builders rest on:
  * Key-point coordinates are pixel indices, so a negative sample coordinate cannot occur in pair scoring: not tested.
  * A line-integral sample a + k (b - a) / 9 of integer end points is never an exact .5 (9 is odd), so ``rint`` against
    Python's ``round`` can differ only at the mid-point (a + b) / 2, which both round half to even; odd sums are in every
    "group" case below.
  * The full-resolution width of an up-sampled map is even, so the last 62-column tile of the column form never holds 1 or 61
    columns; the "full" size cases cover 1 and PTW-1 columns / rows for the square tiles.
  * lwp_set_capacity refuses max_kpts above 1024, so match_kernel's rounds_ok = 0 cannot be reached through the API.
"""
import hashlib

import numpy as np

from oracle import post_ref

KPT = [list(p) for p in post_ref.KPT_IDS]
PAF = [list(p) for p in post_ref.PAF_IDS]
TILES = {0: (16, 32), 1: (32, 32), 2: (16, 64), 3: (32, 64), 4: (32, 62)}     # LWP_PEAK_TILE -> (rows, columns) of a tile
ASSEMBLE_LDS_MAX_ENTRIES = 64 + (60 * 1024) // 160                           # launch_assemble: spill rows in LDS up to here


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _kp(x, y, s, i):
    return (np.int64(x), np.int64(y), np.float32(s), i)


def _number(bt):
    """Give the key-points their running index in type order (the ids group_keypoints expects)."""
    out, n = [], 0
    for l in bt:
        out.append([_kp(x, y, s, n + i) for i, (x, y, s) in enumerate(l)])
        n += len(l)
    return out


def flat_kp(by_type):
    return np.array([[p[0], p[1], p[2], p[3], t] for t, l in enumerate(by_type) for p in l], dtype=np.float64).reshape(-1, 5)


def ychan(limb):
    return PAF[limb][1]


# ------------------------------------------------------------------------------------------------ "group" cases
def _rows(na, nb, xa0=4, xb0=4, dx=1, ya=6, yb=40, sa=0.5, sb=0.6):
    a = [(xa0 + dx * i, ya, sa + 0.001 * i) for i in range(na)]
    b = [(xb0 + dx * j, yb, sb + 0.001 * j) for j in range(nb)]
    return a, b


def _uniform_case(na, nb, caps=None, expect=None, field_to=None):
    """Types 1 and 2 on two rows (1 px apart within a row) under a uniform y field of limb 0, the map high enough that no pair
    is penalised for its length: every one of the na * nb pairs is a candidate.  ``field_to``: the field ends at that column.
    A type 3 key-point below every type 2 one, under a uniform field of limb 2, gives each connection of limb 0 a third part:
    the entries pass the final filter, and their scores (the type 1 scores differ) show WHICH pairs were picked."""
    a, b = _rows(na, nb)
    W = 4 + max(na, nb) + 8
    H = 2 * (W + 40)
    paf = np.zeros((H, W, 38), np.float32)
    paf[:, :field_to, ychan(0)] = 1.0
    paf[:, :, ychan(2)] = 1.0
    bt = [[] for _ in range(18)]
    bt[1], bt[2] = a, b
    bt[3] = [(x, y + 30, 0.7 + 0.001 * j) for j, (x, y, _) in enumerate(b)]
    e = {"cand": {0: na * nb}, "picked": {0: min(na, nb)}}
    e.update(expect or {})
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=caps, expect=e)


def _people_case(P, types_y, limbs, caps=None, expect=None, extra=None, block=0, fill_limbs=()):
    """P people on their own columns (7 px apart); limb l's y field is 1 on the people's columns only, so a limb has exactly P
    candidates (a crossing pair has at most 4 of 10 samples on a column, except 9 columns apart where all ten are: that pair
    is 63 px long in a map 64 high, and the length penalty takes its ratio below zero).  ``block``: the field of ``limbs[0]``
    is also 1 everywhere left of person ``block``: block * block candidates among the first ``block`` people."""
    H, W = 64, 6 + 7 * P + 6
    paf = np.zeros((H, W, 38), np.float32)
    bt = [[] for _ in range(18)]
    for p in range(P):
        x = 5 + 7 * p
        for l in list(limbs) + list(fill_limbs):
            paf[:, x, ychan(l)] = 1.0
        for t, y in types_y:
            bt[t].append((x, y, 0.5 + 0.004 * p))
    if block:
        paf[:, :5 + 7 * (block - 1) + 1, ychan(limbs[0])] = 1.0
    for t, l in (extra or {}).items():
        bt[t] = list(l)
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=caps, expect=expect or {})


def _chain_case(n):
    """n + n key-points under a uniform y field where candidate (A_k, B_k) is beaten at A_k by nothing but at B_k ... by the
    next better one: ratios fall as |dx| grows, and |dx| runs (A0,B0) < (A1,B0) < (A1,B1) < (A2,B1) < ...  The dominant-candidate
    rounds pick one connection per round: n rounds."""
    xa, xb, x = [], [], 6
    for k in range(n):
        xa.append(x)
        x += 2 * k + 1
        xb.append(x)
        x += 2 * k + 2
    H, W = 2 * (x + 40), x + 8
    paf = np.zeros((H, W, 38), np.float32)
    paf[:, :, ychan(0)] = 1.0
    bt = [[] for _ in range(18)]
    paf[:, :, ychan(2)] = 1.0                                  # a third part below every B: the entries pass the filter
    bt[1] = [(v, 6, 0.5 + 0.01 * k) for k, v in enumerate(xa)]
    bt[2] = [(v, 40, 0.6) for v in xb]
    bt[3] = [(v, 70, 0.7) for v in xb]
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=None,
                expect={"cand": {0: n * n}, "picked": {0: n}, "rounds": {0: (">=", n)}})


def _ties_case():
    """Six A and ten B on one column (dx = 0: every pair has ux = 0, uy = 1, ratio exactly 1.0) plus four A on another column:
    100 candidates, 60 of them with the same ratio, so the picks rest on the (i, j) tie-break of the rounds form.  Ten type 3
    key-points further down the column (limb 2: 100 candidates, all with ratio 1.0) make three-part entries that pass the
    filter; the type 1 scores differ, so the entries show which pairs were picked."""
    H, W = 600, 48
    paf = np.zeros((H, W, 38), np.float32)
    paf[:, :, ychan(0)] = 1.0
    paf[:, :, ychan(2)] = 1.0
    bt = [[] for _ in range(18)]
    bt[1] = [(20, 4 + 6 * i, 0.5 + 0.01 * i) for i in range(6)] + [(30, 4 + 6 * i, 0.7) for i in range(4)]
    bt[2] = [(20, 100 + 6 * j, 0.6 + 0.01 * j) for j in range(10)]
    bt[3] = [(20, 200 + 6 * j, 0.7 + 0.01 * j) for j in range(10)]
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=None,
                expect={"cand": {0: 100, 2: 100}, "picked": {0: 10, 2: 10}, "equal_ratio": {0: (">=", 34), 2: (">=", 100)},
                        "entries": 10})


def _scoring_case():
    """Pair scoring next to the map edge and at its decision points, one limb each (types as the COCO limb tables pair them):
    limb 0 (1,2)   the field holds on 9 of 10 samples for one pair and on 8 of 10 for the next, in the last two columns
    limb 2 (2,3)   a pair with equal end points (skipped) beside a regular one
    limb 3 (3,4)   a limb longer than H / 2: the penalty applies
    limb 6 (1,8)   negative fields: a mean that the penalty takes below zero, and a pair of length exactly H / 2 (penalty 0)
    limb 9 (1,11)  the smallest passing samples: a field one float32 above min_paf_score on 9 of 10 samples
    """
    H, W = 128, 96
    paf = np.zeros((H, W, 38), np.float32)
    bt = [[] for _ in range(18)]
    # limb 0: vertical pairs in columns W-1 and W-2, rows 0 .. 36 (samples every 4 rows): the field ends after sample 8 / 7
    bt[1] = [(W - 1, 0, 0.9), (W - 2, 0, 0.8), (0, 127, 0.7)]
    bt[2] = [(W - 1, 36, 0.9), (W - 2, 36, 0.8), (0, 127, 0.6)]
    paf[0:33, W - 1, ychan(0)] = 1.0            # samples at rows 0, 4, .., 32 pass: 9 of 10
    paf[0:29, W - 2, ychan(0)] = 1.0            # rows 0 .. 28: 8 of 10
    # limb 2: type 2 #2 and type 3 #0 share a pixel (0, 127), the bottom-left corner; type 3 #1 continues pair 0 along column W-1
    bt[3] = [(0, 127, 0.5), (W - 1, 60, 0.7)]
    paf[30:64, W - 1, ychan(2)] = 1.0
    # limb 3: (3,4) from (W-1, 60) up to row 127 is 67 px > H / 2 = 64: penalty 64 / 67 - 1
    bt[4] = [(W - 1, 127, 0.7)]
    paf[56:128, W - 1, ychan(3)] = 1.0
    # limb 6: (1,8) from type 1 #2 (0,127) straight up to (0, 0): uy = -1 on a field of -0.5, norm 127 > 64: the mean 0.5 and
    # the penalty 64 / 127 - 1 leave a ratio of 0.0039, a candidate; and from type 1 #0 (W-1, 0) along row 0 to (W-1-64, 0):
    # norm 64 = H / 2, penalty min(0, 0) = 0, x field -0.25 against ux = -1: ratio 0.25  (ratio exactly 0: _ratio_zero_case)
    bt[8] = [(0, 0, 0.6), (W - 1 - 64, 0, 0.6)]
    paf[:, 0, ychan(6)] = -0.5
    paf[0, :, PAF[6][0]] = -0.25
    # limb 9: (1,11): type 1 #1 (W-2, 0) down column W-2: field nextafter(0.05f) on 9 samples: the smallest passing ratio
    bt[11] = [(W - 2, 18, 0.5)]
    paf[0:17, W - 2, ychan(9)] = np.nextafter(np.float32(0.05), np.float32(1))
    # limb 0's statement: the 9-of-10 pair (0, 0) is a candidate, the 8-of-10 pair (1, 1) is not (with rounded samples the
    # crossing pair (1, 0) has 9 samples on the field too: 1 candidate under demo, 2 otherwise)
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=None,
                expect={"cand": {0: ("in", 1, 2), 2: 1, 3: 1}, "penalised": 3, "has": {0: [(0, 0)]}, "lacks": {0: [(1, 1)]}})


def _ratio_zero_case():
    """``ratio > 0`` at its edge.  The map is 65 high (height_n = 32) and every pair runs down a column from row 0 to row 64:
    norm 64 = 2 height_n, so the penalty is 32 / 64 - 1 = -0.5 exactly, uy = 1, and all ten samples see the column's field f:
    the mean is (10 f) / 10 = f exactly for these f, the ratio f - 0.5.
      pair (0, 0)  f = 0.5                    ratio exactly 0.0: not a candidate
      pair (1, 1)  f = nextafter(0.5f, 1)     ratio 2^-24 = 5.96e-8: a candidate, the smallest positive ratio this geometry has
      pair (2, 2)  f = nextafter(0.5f, 0)     ratio -2^-25: not a candidate
    The smallest positive double (4.9e-324) cannot be reached: a ratio is a mean of float32-valued samples plus a quotient of
    small integers, and the differences of such numbers are nowhere near the subnormal range."""
    H, W = 65, 64
    paf = np.zeros((H, W, 38), np.float32)
    half = np.float32(0.5)
    fields = (half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)))
    bt = [[] for _ in range(18)]
    for k, f in enumerate(fields):
        x = 10 + 20 * k
        paf[:, x, ychan(0)] = f
        bt[1].append((x, 0, 0.9))
        bt[2].append((x, 64, 0.8))
        bt[3].append((x + 3, 64, 0.7))          # a third part along row 64 (limb 2, x field): the one accepted pair's entry survives
    paf[64, :, PAF[2][0]] = 1.0
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=None,
                expect={"cand": {0: 1}, "has": {0: [(1, 1)]}, "lacks": {0: [(0, 0), (2, 2)]}, "ratio": {0: {(1, 1): 2.0 ** -24}}, "entries": 1})


def _unbound_case(passing_first):
    H, W = 64, 64
    paf = np.zeros((H, W, 38), np.float32)
    paf[:, :, ychan(0)] = 1.0
    paf[25, 40, PAF[0][0]] = np.nan                 # the mid-point of the pair at x = 40
    bt = [[] for _ in range(18)]
    xs = (20, 40) if passing_first else (40, 20)
    bt[1] = [(x, 10, 0.9) for x in xs]
    bt[2] = [(x, 40, 0.8) for x in xs]
    bt[3] = [(x, 60, 0.7) for x in xs]
    paf[:, :, ychan(2)] = 1.0
    return dict(kind="group", by_type=_number(bt), paf=paf, caps=None, expect={"raises": None if passing_first else "unbound"})


def group_cases():
    c = {}
    # ---- match_kernel: the count of candidates m against 64 and 1024, min(na, nb) against 64
    c["m64_8x8"] = _uniform_case(8, 8)                                              # register form, full
    c["m65_5x13"] = _uniform_case(5, 13)                                            # rounds form, one over
    # na = 65 with m <= 64: no register form
    c["m_le64_na65_nb1"] = _uniform_case(65, 1, field_to=40, expect={"cand": {0: ("in", 1, 64)}, "kpts": {1: 65, 2: 1}})
    # scan form, want = 65
    c["m65_65x65"] = _people_case(65, [(1, 10), (2, 30), (3, 50)], [0, 2], expect={"cand": {0: 65}, "picked": {0: 65}, "entries": 65})
    c["m1024_32x32"] = _uniform_case(32, 32)                                        # rounds form, LDS full
    c["m1025_25x41"] = _uniform_case(25, 41)                                        # scan form from global memory
    # min(na, nb) = 64: rounds form; 65: scan form from LDS
    c["want64_rounds"] = _people_case(64, [(1, 10), (2, 30), (3, 50)], [0, 2], block=8,
                                      expect={"cand": {0: ("in", 65, 1024)}, "picked": {0: 64}, "entries": 64})
    c["want65_scan"] = _people_case(65, [(1, 10), (2, 30), (3, 50)], [0, 2], block=8,
                                    expect={"cand": {0: ("in", 65, 1024)}, "picked": {0: 65}, "entries": 65})
    c["m4096_max_conn"] = _uniform_case(64, 64)                                     # m = max_conn: scan form, nothing dropped
    c["m1024_cap1024"] = _uniform_case(32, 32, caps=dict(max_conn=1024))
    c["m1025_cap1024"] = _uniform_case(25, 41, caps=dict(max_conn=1024), expect={"raises": "capacity"})
    c["ties_60_of_100"] = _ties_case()
    c["chain_9_rounds"] = _chain_case(9)
    # ---- assemble_kernel: surviving entries against 64 (lane registers / spilled rows), LDS spill and global scratch
    body = [(1, 8), (2, 20), (3, 32), (16, 44)]                 # neck, shoulder, elbow on limbs 0 and 2; limb 17 (2 -> 16) fills the ear
    for P in (63, 64, 65):
        # (limb 14 (14 -> 16) is one-sided, no type 14, with P key-points of type 16 that no entry holds yet: P more entries
        # behind the first P, 2 P in all, dropped by the filter; limb 17 then fills the ear of the first P)
        ex = {"picked": {0: P, 2: P, 17: P}, "entries": P, "entries_before_filter": 2 * P}
        c["entries%d" % P] = _people_case(P, body, [0, 2], fill_limbs=[17], expect=ex)
        c["entries%d_global" % P] = _people_case(P, body, [0, 2], fill_limbs=[17], expect=ex,
                                                 caps=dict(max_entries=ASSEMBLE_LDS_MAX_ENTRIES + 1))
    c["entries65_lds_limit"] = _people_case(65, body, [0, 2], fill_limbs=[17], caps=dict(max_entries=ASSEMBLE_LDS_MAX_ENTRIES),
                                            expect={"picked": {0: 65, 2: 65, 17: 65}, "entries": 65})
    # one-sided limbs 7 (8 -> 9, no type 9), 14 (-> 16) and 16 (-> 17) with 65 key-points each that no entry holds, behind 65
    # entries: 195 more entries (indices 65 .. 259) that the filter drops, 260 in all, so the case runs at max_entries = 300;
    # limb 18 (5 -> 17) fills the ear of the entries that limb 1 (1 -> 5) gave a type 5
    far = [(5 + 7 * p, 60, 0.4) for p in range(65)]
    c["one_sided_65_behind_65"] = _people_case(65, body + [(5, 14), (17, 26)], [0, 2, 1], fill_limbs=[17, 18], extra={8: far},
                                               caps=dict(max_entries=300),
                                               expect={"picked": {0: 65, 1: 65, 2: 65, 17: 65, 18: 65}, "entries": 65,
                                                       "entries_before_filter": 260})
    c["entries_cap70_70"] = _people_case(70, body[:3], [0, 2], caps=dict(max_entries=70),
                                         expect={"entries": 70, "entries_before_filter": 70})
    c["entries_cap70_71"] = _people_case(71, body[:3], [0, 2], caps=dict(max_entries=70), expect={"raises": "capacity"})
    # ---- pair scoring at the map edge and its decision points; the reference's latent UnboundLocalError
    c["scoring_edges"] = _scoring_case()
    c["ratio_zero"] = _ratio_zero_case()
    c["unbound_first_pair"] = _unbound_case(False)
    c["unbound_after_passing_pair"] = _unbound_case(True)
    return c


# ------------------------------------------------------------------------------------------------ "full" cases
def _spikes(H, W, per_type):
    heat = np.zeros((H, W, 19), np.float32)
    for t, pts in per_type.items():
        for k, (x, y) in enumerate(pts):
            heat[y, x, t] = np.float32(0.3 + 0.6 * ((k * 37) % 101) / 101.0)
    return heat


def _isolated(n, W, x0=3, y0=3, step=7):
    per_row = (W - x0 - 1) // step + 1
    return [(x0 + step * (k % per_row), y0 + step * (k // per_row)) for k in range(n)]


def _full_nms_case():
    """One type per count or arrangement of nms_kernel (128 x 192, spikes of distinct heights)."""
    H, W = 128, 192
    t = {}
    for ty, n in enumerate((63, 64, 65, 127, 128)):              # isolated spikes: peaks = key-points = n (128 = max_kpts)
        t[ty] = _isolated(n, W)
    t[5] = _isolated(128, W) + [(3 + 2, 3)]                       # 129 peaks, one 2 px from the first: 128 kept
    t[6] = [(10, 10), (15, 10), (20, 10),                         # A - 5 - B - 5 - C: A drops B, C survives (10 from A)
            (40, 10), (40, 15), (40, 20),                         # the same along y at equal x
            (60, 10), (66, 10), (60, 30), (60, 36),               # distance exactly 6: kept (the test is < 36)
            (80, 10), (85, 13), (100, 10), (103, 15)]             # 34 < 36 dropped; 34 again with the larger share in y
    t[7] = [(47, 2 * k) for k in range(40)] + [(50, 2 * k) for k in range(60)]   # 100 peaks on two columns 3 px apart: the LDS form's
    #                                                                             64-wide sweep window splits column 50
    t[8] = [(x, y) for x in range(20, 52, 2) for y in range(20, 52, 2)]          # 256 = a power of two
    t[9] = t[8] + [(60, 60)]                                                      # ... and one more
    # R = 1 tile seams of every geometry, the image border and its corners
    t[10] = [(x, y) for x in (0, 31, 63, 95, 127, 159, 191) for y in (0, 15, 31, 47, 63, 95, 127)]
    t[11] = [(x, y) for x in (32, 64, 96, 128, 160) for y in (16, 32, 48, 64, 96)]
    t[12] = [(61, 8), (62, 20), (123, 8), (124, 20), (185, 8), (186, 20)]
    for ty in range(13, 18):                                      # no empty type: a limb with one empty side would seed an entry per
        t[ty] = [(5, 5)]                                          # key-point of the other (hundreds here, past max_entries)
    e = {"peaks": {0: 63, 1: 64, 2: 65, 3: 127, 4: 128, 5: 129, 7: 100, 8: 256, 9: 257}, "kpts": {0: 63, 1: 64, 2: 65, 3: 127, 4: 128, 5: 128}}
    return dict(kind="full", heat=_spikes(H, W, t), caps=None, expect=e)


def _full_size_case(H, W):
    """Spikes on the border, the corners and both sides of every tile seam of a small map."""
    xs = sorted({x for x in (0, 1, 15, 16, 31, 32, 61, 62, 63, 64, W - 2, W - 1) if 0 <= x < W})
    ys = sorted({y for y in (0, 1, 15, 16, 31, 32, H - 2, H - 1) if 0 <= y < H})
    t = {}
    for ty in range(4):                                        # 4 types: the (x + y) % 4 classes, so that no two spikes touch
        t[ty] = [(x, y) for x in xs for y in ys if (x + 2 * y) % 4 == ty]
    t[4] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
    n = sum(len(v) for v in t.values())
    return dict(kind="full", heat=_spikes(H, W, t), caps=None, expect={"total_peaks": n})


def _full_capacity(n_iso, caps, raises, extra=()):
    H, W = 128, 192
    t = {0: _isolated(n_iso, W) + list(extra)}
    e = {"peaks": {0: n_iso + len(extra)}}
    if raises:
        e["raises"] = "capacity"
    return dict(kind="full", heat=_spikes(H, W, t), caps=caps, expect=e)


def full_cases():
    c = {"nms_counts": _full_nms_case()}
    for H, W in ((10, 20), (16, 32), (32, 64), (33, 65), (47, 95), (63, 127)):   # below one tile, exactly one, 1 and PT-1 in the last
        c["size_%dx%d" % (H, W)] = _full_size_case(H, W)
    c["kept129_cap128"] = _full_capacity(129, None, True)                         # kept = max_kpts + 1: an error, no truncation
    dense = [(x, y) for x in range(100, 132, 2) for y in range(90, 118, 2)]       # 224 peaks 2 px apart
    c["peaks256_cap256"] = _full_capacity(32, dict(max_peaks=256), False, dense)
    c["peaks257_cap256"] = _full_capacity(33, dict(max_peaks=256), True, dense)
    return c


# ------------------------------------------------------------------------------------------------ "maps" cases
def bump_weights(R):
    """Per sub-pixel phase p in 0..R-1: a neighbour offset (-1 / +1) and a weight a such that the low-resolution pair
    (1 at c, a at c + offset) has its strict maximum at full-resolution index c * R + p after the cubic up-sampling (searched
    with the oracle's float32 tables)."""
    out = {}
    for off in (1, -1):
        for a in np.linspace(0.02, 0.98, 49).astype(np.float32):
            row = np.zeros((1, 9, 1), np.float32)
            row[0, 4, 0], row[0, 4 + off, 0] = 1.0, a
            up = post_ref.upsample_cubic(row, R)[0 if R == 1 else R // 2, :, 0]
            m = int(np.argmax(up))
            if (up == up[m]).sum() == 1 and 4 * R <= m < 5 * R:
                out.setdefault(m - 4 * R, (off, np.float32(a)))
    return out


def _place(heat, t, R, x, y, amp, wts):
    """A bump of type t whose maximum is the full-resolution pixel (x, y)."""
    cx, cy = x // R, y // R
    ox, ax = wts[x % R]
    oy, ay = wts[y % R]
    h, w = heat.shape[1:]
    # on the image border no neighbour is needed: the replicated edge overshoots towards the last pixel, which is the maximum
    if x in (0, w * R - 1):
        ox, ax = 0, np.float32(1)
    if y in (0, h * R - 1):
        oy, ay = 0, np.float32(1)
    if not (0 <= cx + ox < w and 0 <= cy + oy < h):
        return False
    if heat[t, max(cy - 2, 0):cy + 3, max(cx - 2, 0):cx + 3].any():
        return False
    heat[t, cy, cx] = amp
    heat[t, cy, cx + ox] = amp * ax
    heat[t, cy + oy, cx] = amp * ay
    heat[t, cy + oy, cx + ox] = amp * ax * ay
    return True


def _seam_targets(Hf, Wf):
    xs = {0, Wf - 1}
    ys = {0, Hf - 1}
    for _, (th, tw) in TILES.items():
        xs |= {x for s in range(tw, Wf, tw) for x in (s - 1, s)}
        ys |= {y for s in range(th, Hf, th) for y in (s - 1, s)}
    return sorted(xs), sorted(ys)


def _maps_seams(h, w, R, seed):
    """Bumps whose maxima sit on the first / last column and row of the tiles of every geometry, on the image border, and on
    every sub-pixel phase; a plateau over a seam; values around the 0.1 threshold; NaN / inf pixels beside a seam."""
    rng = np.random.RandomState(seed)
    wts = bump_weights(R)
    assert sorted(wts) == list(range(R)), sorted(wts)
    heat = np.zeros((19, h, w), np.float32)
    Hf, Wf = h * R, w * R
    xs, ys = _seam_targets(Hf, Wf)
    targets = [(x, int(rng.randint(0, Hf))) for x in xs] + [(int(rng.randint(0, Wf)), y) for y in ys]
    targets += [(x, y) for x in xs[:6] for y in ys[:4]] + [(0, 0), (Wf - 1, 0), (0, Hf - 1), (Wf - 1, Hf - 1)]
    targets += [(int(rng.randint(0, Wf)) // R * R + p, int(rng.randint(0, Hf)) // R * R + q) for p in range(R) for q in range(R)]
    for k, (x, y) in enumerate(targets):          # (aimed at: beside the image border the replicated edge can move a maximum by a pixel)
        for t in range(12):
            tt = (k + t) % 12
            if _place(heat, tt, R, x, y, np.float32(0.4 + 0.5 * rng.rand()), wts):
                break
    extras = h >= 16 and 64 // R + 4 < w
    if extras:
        # type 12: two equal low-resolution pixels across the seams at x = 32 and x = 124 (the two full-resolution pixels beside
        # the seam are equal in float32: no strict maximum, no key-point)
        for cx in (32 // R - 1, 124 // R - 1):
            if cx + 1 < w:
                heat[12, 5, cx] = heat[12, 5, cx + 1] = 0.7
        # type 13: amplitudes that interpolate to just below, exactly at and just above 0.1f (searched in float32: consecutive
        # float32 amplitudes), at THRESHOLD_CELLS in that order; negative overshoot around a large bump
        for (cx, cy), amp in zip(THRESHOLD_CELLS + ((4, 12),), threshold_amplitudes(R, wts) + (np.float32(0.95),)):
            assert _place(heat, 13, R, cx * R + R // 2, cy * R + R // 2, amp, wts)
        # type 14 / 15: a NaN and a +inf pixel next to the seam at x = 64 (62 for the column form), a bump three pixels away
        # (the poisoned 4 x 4 footprint reaches its halo)
        heat[14, 6, 64 // R] = np.nan
        heat[15, 14, 64 // R - 1] = np.inf
        for t, cy in ((14, 6), (15, 14)):
            assert _place(heat, t, R, (64 // R + 3) * R + R // 2, cy * R + R // 2, np.float32(0.8), wts)
    paf = np.zeros((38, h, w), np.float32)
    for l in range(19):
        paf[PAF[l][1]] = 0.3
    return dict(kind="maps", heat=heat, paf=paf, ratio=R, caps=None, expect={"seams": 1, "extras": extras})


THRESHOLD_CELLS = ((4, 4), (12, 4), (12, 12))       # low-resolution cells of the below / at / above bumps of type 13


def threshold_amplitudes(R, wts):
    """Three float32 bump amplitudes: the largest whose up-sampled maximum is below 0.1f, the next float32 (its maximum must
    be exactly 0.1f, asserted: the `<` against `<=` edge of the threshold), and the smallest whose maximum is above 0.1f."""
    def top(a):
        m = np.zeros((1, 9, 9), np.float32)
        _place(m, 0, R, 4 * R + R // 2, 4 * R + R // 2, np.float32(a), wts)
        return post_ref.upsample_cubic(m.transpose(1, 2, 0), R).max()
    thr = np.float32(0.1)
    lo, hi = np.float32(0.05), np.float32(0.2)
    assert top(lo) < thr <= top(hi)
    while np.nextafter(lo, hi) < hi:
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if top(mid) < thr:
            lo = mid
        else:
            hi = mid
    assert top(lo) < thr and top(hi) == thr, (top(lo), top(hi))
    above = np.nextafter(hi, np.float32(1))
    while not top(above) > thr:
        above = np.nextafter(above, np.float32(1))
    return lo, hi, above


PAIR_COUNTS = {0: 16, 1: 5, 2: 4, 3: 1, 4: 1, 5: 1, 6: 6, 9: 19, 10: 1, 11: 7, 12: 3, 13: 107, 14: 20, 15: 11, 17: 29}
PAIR_PRODUCTS = {3: 1, 2: 4, 1: 5, 4: 6, 8: 19, 0: 20, 10: 21, 16: 319, 13: 320, 11: 321}     # limb -> na * nb


def _maps_pairs(h, w, R, seed):
    """Key-point counts per type chosen so that the limbs' na * nb are 1, 4, 5, 6, 19, 20, 21, 319, 320, 321 (5 pairs per
    wave, 20 per workgroup, 320 per grid iteration of score_pairs_kernel), the key-points spread over the whole map with the
    outer two low-resolution columns and rows first: their samples take sample_map_rows' scalar footprint, the interior ones
    the row form, and pairs between them mix both."""
    rng = np.random.RandomState(seed)
    heat = np.zeros((19, h, w), np.float32)
    border = [(x, y) for x in (0, 1, w - 2, w - 1) for y in range(0, h, 3)] + [(x, y) for y in (0, 1, h - 2, h - 1) for x in range(2, w - 2, 3)]
    for t, n in PAIR_COUNTS.items():
        cells = [border[i] for i in rng.permutation(len(border))] + [(int(rng.randint(2, w - 2)), int(rng.randint(2, h - 2))) for _ in range(4000)]
        placed = 0
        for cx, cy in cells:
            if placed == n:
                break
            if heat[t, max(cy - 2, 0):cy + 3, max(cx - 2, 0):cx + 3].any():
                continue
            heat[t, cy, cx] = np.float32(0.4 + 0.5 * rng.rand())
            ox = 1 if cx + 2 < w else -1              # the weaker neighbour on the inner side: next to the replicated border it
            oy = 1 if cy + 2 < h else -1              # would raise a second, lower maximum on the border itself
            heat[t, cy, cx + ox] = heat[t, cy, cx] * np.float32(0.5)
            heat[t, cy + oy, cx] = heat[t, cy, cx] * np.float32(0.25)
            heat[t, cy + oy, cx + ox] = heat[t, cy, cx] * np.float32(0.125)
            placed += 1
        assert placed == n, (t, placed)
    paf = (0.25 + 0.02 * rng.randn(38, h, w)).astype(np.float32)
    paf[:, h // 2:, :] *= np.float32(0.15)                  # lower half: samples on both sides of min_paf_score
    return dict(kind="maps", heat=heat, paf=paf, ratio=R, caps=None,
                expect={"kpts": dict(PAIR_COUNTS), "pairs": dict(PAIR_PRODUCTS), "border_kpts": (">=", 40)})


def maps_cases():
    return {"seams_r4": _maps_seams(46, 82, 4, 1), "seams_r8": _maps_seams(24, 40, 8, 2), "seams_r4_one_tile": _maps_seams(8, 16, 4, 3),
            "seams_r4_small": _maps_seams(6, 10, 4, 4), "pairs_r4": _maps_pairs(46, 82, 4, 5), "pairs_r8": _maps_pairs(40, 60, 8, 6)}


def other_frames(case, n=2):
    """n different maps of the case's shape (the other frames of a batch)."""
    rng = np.random.RandomState(99)
    out = []
    for _ in range(n):
        hh = np.zeros_like(case["heat"])
        flat = hh.reshape(-1)
        flat[rng.choice(flat.size, size=max(4, flat.size // 400), replace=False)] = 0.6
        out.append(hh)
    return out


def all_cases():
    out = {}
    for kind, fn in (("group", group_cases), ("full", full_cases), ("maps", maps_cases)):
        for name, c in fn().items():
            out["%s/%s" % (kind, name)] = c
    return out


def input_digest(case):
    if case["kind"] == "group":
        return digest(flat_kp(case["by_type"])) + digest(case["paf"])
    if case["kind"] == "full":
        return digest(case["heat"])
    return digest(case["heat"]) + digest(case["paf"])


# ------------------------------------------------------------------------------------------------ the oracle on a case
def run_oracle(case, demo, mod=post_ref, with_counts=True):
    """The case through ``mod``'s extract_keypoints / group_keypoints (the oracle, or the reference's module in the generator).
    Returns dict(kp (n,5), entries, allk, heat_mut (full only), counts (oracle only))."""
    counts = {} if with_counts else None
    kw = dict(counts=counts) if with_counts else {}
    if case["kind"] == "group":
        bt = [list(l) for l in case["by_type"]]
        ent, allk = mod.group_keypoints(bt, case["paf"], demo=demo, **kw)
        if with_counts:
            counts["kpts"] = [len(l) for l in bt]
        return dict(kp=flat_kp(bt), entries=np.asarray(ent, dtype=np.float64), allk=np.asarray(allk, dtype=np.float64), counts=counts)
    if case["kind"] == "full":
        hu = case["heat"].copy()
        pu = np.zeros(hu.shape[:2] + (38,), np.float32)
    else:
        hu = post_ref.upsample_cubic(case["heat"].transpose(1, 2, 0), case["ratio"])
        pu = post_ref.upsample_cubic(case["paf"].transpose(1, 2, 0), case["ratio"])
    by_type, total = [], 0
    for k in range(18):
        total += mod.extract_keypoints(hu[:, :, k], by_type, total, **kw)
    ent, allk = mod.group_keypoints(by_type, pu, demo=demo, **kw)
    return dict(kp=flat_kp(by_type), entries=np.asarray(ent, dtype=np.float64), allk=np.asarray(allk, dtype=np.float64),
                heat_mut=hu, counts=counts)


def rounds_needed(cands):
    """Rounds of the dominant-candidate form of match_kernel on a candidate list [i, j, ratio, ..] (scoring order)."""
    live = [(-c[2], c[0], c[1]) for c in cands]
    rounds = 0
    while live:
        rounds += 1
        best_a, best_b = {}, {}
        for c in live:
            best_a[c[1]] = min(best_a.get(c[1], c), c)
            best_b[c[2]] = min(best_b.get(c[2], c), c)
        picks = [c for c in live if best_a[c[1]] == c and best_b[c[2]] == c]
        ua, ub = {c[1] for c in picks}, {c[2] for c in picks}
        live = [c for c in live if c[1] not in ua and c[2] not in ub]
    return rounds


def _cmp(got, want):
    if isinstance(want, tuple):
        if want[0] == "in":
            return want[1] <= got <= want[2]
        return got >= want[1]
    return got == want


def check_expect(case, res):
    """Assert the case's boundary statement on the oracle's result ``res`` (run_oracle, demo either way).  ``raises`` cases
    state what the library must report; their counts are checked as far as the oracle gets."""
    e, cnt = case["expect"], res["counts"]
    kp = res["kp"]
    for key in ("peaks", "kpts", "cand", "picked"):
        for idx, want in e.get(key, {}).items():
            assert _cmp(cnt[key][idx], want), (key, idx, cnt[key][idx], want)
    if "entries" in e:
        assert len(res["entries"]) == e["entries"], len(res["entries"])
    if case["kind"] == "group" and not e.get("raises"):
        assert len(res["entries"]) >= 1, "no entry passes the filter: the picks would be invisible"
    if "entries_before_filter" in e:
        assert cnt["entries_before_filter"] == e["entries_before_filter"], cnt["entries_before_filter"]
    for limb, want in e.get("rounds", {}).items():
        assert _cmp(rounds_needed(cnt["cands"][limb]), want), (limb, rounds_needed(cnt["cands"][limb]))
    for limb, want in e.get("equal_ratio", {}).items():
        r = [c[2] for c in cnt["cands"][limb]]
        assert _cmp(max(r.count(v) for v in set(r)), want), limb
        assert 65 <= len(r) <= 1024
    for limb, want in e.get("pairs", {}).items():
        a, b = KPT[limb]
        assert cnt["kpts"][a] * cnt["kpts"][b] == want, (limb, cnt["kpts"][a], cnt["kpts"][b])
    if "total_peaks" in e:
        assert sum(cnt["peaks"]) == e["total_peaks"], sum(cnt["peaks"])
    for limb, pairs in e.get("has", {}).items():
        got = {(c[0], c[1]) for c in cnt["cands"][limb]}
        assert set(pairs) <= got, (limb, pairs, sorted(got))
    for limb, pairs in e.get("lacks", {}).items():
        got = {(c[0], c[1]) for c in cnt["cands"][limb]}
        assert not set(pairs) & got, (limb, pairs, sorted(got))
    for limb, want in e.get("ratio", {}).items():
        got = {(c[0], c[1]): c[2] for c in cnt["cands"][limb]}
        for ij, r in want.items():
            assert got[ij] == r, (limb, ij, got[ij], r)
    if "penalised" in e:
        limb = e["penalised"]
        assert any(c[2] < 1.0 for c in cnt["cands"][limb]), cnt["cands"][limb]
    if "border_kpts" in e:
        H, W = res["heat_mut"].shape[:2]
        R = case["ratio"]
        edge = (kp[:, 0] < 2 * R) | (kp[:, 0] >= W - 2 * R) | (kp[:, 1] < 2 * R) | (kp[:, 1] >= H - 2 * R)
        assert _cmp(int(edge.sum()), e["border_kpts"]), int(edge.sum())
    if "seams" in e:
        H, W = res["heat_mut"].shape[:2]
        for sel, (th, tw) in TILES.items():
            x, y = kp[:, 0].astype(int), kp[:, 1].astype(int)
            if W >= 2 * tw:                                         # (a seam the image border does not reach)
                assert ((x % tw == 0) & (x > 0)).sum() >= 1 and (x % tw == tw - 1).sum() >= 1, (sel, "columns")
            if H >= 2 * th:
                assert ((y % th == 0) & (y > 0)).sum() >= 1 and (y % th == th - 1).sum() >= 1, (sel, "rows")
        # maxima on the image border: at ratio 4 the replicated edge overshoots up to the outermost pixel; at ratio 8 the cubic's
        # overshoot peaks one pixel inside it (frac 0.6875), whatever the neighbours hold
        b = 0 if case["ratio"] == 4 else 1
        assert (kp[:, 0] == b).any() and (kp[:, 0] == W - 1 - b).any() and (kp[:, 1] == b).any() and (kp[:, 1] == H - 1 - b).any()
        if e["extras"]:
            assert not (kp[:, 4] == 12).any(), kp[kp[:, 4] == 12]        # the plateaus over a seam yield no key-point
            # type 13: the bump just below 0.1f yields no key-point, the one at exactly 0.1f and the one above do (+ the large one)
            R, thr = case["ratio"], np.float32(0.1)
            t13 = {(int(r[0]) // R, int(r[1]) // R): np.float32(r[2]) for r in kp[kp[:, 4] == 13]}
            below, at, above = THRESHOLD_CELLS
            assert len(t13) == 3 and below not in t13, t13
            assert t13[at] == thr, t13[at]
            assert thr < t13[above] <= np.nextafter(np.nextafter(thr, np.float32(1)), np.float32(1)), t13[above]
            assert np.isnan(res["heat_mut"][:, :, 14]).any() and np.isinf(res["heat_mut"][:, :, 15]).any()
