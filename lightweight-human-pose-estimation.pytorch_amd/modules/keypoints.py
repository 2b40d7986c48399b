"""Drop-ins for the reference's ``modules.keypoints`` (modules/keypoints.py:5-201), running on the GPU.

``extract_keypoints`` and ``group_keypoints`` keep the reference's signatures and conventions:
in-place thresholding of the heat-map, append-to-caller's-list out-parameter, tuples of
(np.int64 x, np.int64 y, np.float32 score, int id), float64 (P,pose_entry_size)/(K,4) results, ``(0,)``-shaped
empties.  The computation is HIP kernels behind the C ABI (lwp_extract_keypoints / lwp_group_keypoints).
``group_keypoints`` reads BODY_PARTS_KPT_IDS / BODY_PARTS_PAF_IDS of this module at call time, as the reference does
(TRAIN-ON-CUSTOM-DATASET.md): set them for a custom key-point set; the engine's skeleton follows (lwp_set_skeleton).
"""
import numpy as np

from ..runtime import default_engine

BODY_PARTS_KPT_IDS = [[1, 2], [1, 5], [2, 3], [3, 4], [5, 6], [6, 7], [1, 8], [8, 9], [9, 10], [1, 11],
                      [11, 12], [12, 13], [1, 0], [0, 14], [14, 16], [0, 15], [15, 17], [2, 16], [5, 17]]
BODY_PARTS_PAF_IDS = ([12, 13], [20, 21], [14, 15], [16, 17], [22, 23], [24, 25], [0, 1], [2, 3], [4, 5],
                      [6, 7], [8, 9], [10, 11], [28, 29], [30, 31], [34, 35], [32, 33], [36, 37], [18, 19], [26, 27])


def extract_keypoints(heatmap, all_keypoints, total_keypoint_num, engine=None):
    eng = engine or default_engine()
    xs, ys, sc = eng.extract_keypoints(heatmap)
    found = [(xs[i], ys[i], sc[i], total_keypoint_num + i) for i in range(len(xs))]
    all_keypoints.append(found)
    return len(found)


def _skeleton_args(K, pose_entry_size, min_paf_score):
    """This module's tables, read at call time like the reference (modules/keypoints.py:54-61), checked where no engine is needed."""
    paf_ids = [[int(c) for c in p] for p in BODY_PARTS_PAF_IDS]
    kpt_ids = [[int(t) for t in p] for p in BODY_PARTS_KPT_IDS]
    L = len(paf_ids)
    if not 1 <= K <= 64:
        raise ValueError("the HIP path groups 1..64 key-point types, got %d" % K)
    if not 1 <= L <= 320:
        raise ValueError("BODY_PARTS_PAF_IDS must list 1..320 limbs, got %d" % L)
    if len(kpt_ids) < L:
        raise ValueError("BODY_PARTS_KPT_IDS has %d limbs, BODY_PARTS_PAF_IDS %d" % (len(kpt_ids), L))
    kpt_ids = kpt_ids[:L]
    for l, ((a, b), pc) in enumerate(zip(kpt_ids, paf_ids)):
        if not (0 <= a < K and 0 <= b < K) or a == b:
            raise ValueError("limb %d: key-point types (%d, %d) must be distinct and in 0..%d" % (l, a, b, K - 1))
        if len(pc) != 2 or min(pc) < 0:
            raise ValueError("limb %d: bad PAF channel pair %r" % (l, pc))
    if int(pose_entry_size) != pose_entry_size or not K + 2 <= pose_entry_size <= 256:
        raise ValueError("pose_entry_size must be an integer in K + 2 = %d .. 256 (the reference would overwrite key-point "
                         "columns with the score and count), got %r" % (K + 2, pose_entry_size))
    return K, kpt_ids, paf_ids, int(pose_entry_size), float(min_paf_score)


def group_keypoints(all_keypoints_by_type, pafs, pose_entry_size=20, min_paf_score=0.05, demo=False, engine=None):
    K, kpt_ids, paf_ids, E, mp = _skeleton_args(len(all_keypoints_by_type), pose_entry_size, min_paf_score)
    eng = engine or default_engine()
    sk = eng.skeleton
    cur = (sk["num_kpt_types"], sk["limb_kpts"].tolist(), sk["limb_pafs"].tolist(), sk["pose_entry_size"], sk["min_paf_score"])
    if cur != (K, kpt_ids, paf_ids, E, mp):     # pushed only when it changed (the engine re-sizes its workspaces)
        eng.set_skeleton(kpt_ids, paf_ids, K, E, mp)
    all_keypoints = np.array([item for sublist in all_keypoints_by_type for item in sublist])
    counts = np.array([len(s) for s in all_keypoints_by_type], dtype=np.int32)
    kp = all_keypoints.reshape(-1, 4) if all_keypoints.size else np.zeros((0, 4))
    entries = eng.group_keypoints(kp, counts, pafs, demo)
    pose_entries = entries if len(entries) else np.asarray([])
    return pose_entries, all_keypoints
