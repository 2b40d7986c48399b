"""Shared by test_val_device_host.py and test_gpu_val_device.py: a NumPy statement of the append kernel (coco_append_kernel,
csrc/eval_kernels.hip), the golden frames it is pinned on, and the edge frames of the rows test.  A frame is what
``Engine.poses_from_maps`` returns for one image: pose entries (P, 20) float64 (18 key-point ids or -1, the score, the count)
and key-point rows (n, 4) float64 (x, y, score, id), compact and in id order."""
import json
import os

import numpy as np

from conftest import GOLDEN

# slot of each of the 18 network key-points in COCO's order (val.py:59); the neck, type 1, has none
TO_COCO = [0, -1, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3]


def append_rows(entries, allk):
    """What the append kernel writes for one frame: (keypoints (P, 17, 3), scores (P,)) float64, operation by operation."""
    entries = np.asarray(entries, dtype=np.float64).reshape(-1, 20)
    allk = np.asarray(allk, dtype=np.float64).reshape(-1, 4)
    kp = np.zeros((len(entries), 17, 3), dtype=np.float64)
    score = np.zeros(len(entries), dtype=np.float64)
    for e, row in enumerate(entries):
        for t in range(18):
            if TO_COCO[t] < 0 or row[t] == -1.0:
                continue
            r = int(row[t])
            kp[e, TO_COCO[t]] = (allk[r, 0] + np.float64(0.5), allk[r, 1] + np.float64(0.5), 1.0)
        m = row[19] - np.float64(1.0)
        score[e] = row[18] * (m if m > 0.0 else np.float64(0.0))
    return kp, score


def golden_frames():
    """name -> (entries, key-points) of every golden frame that holds poses (tests/golden/post_*.npz, coco_format.json)."""
    with open(os.path.join(GOLDEN, "coco_format.json")) as f:
        names = sorted(json.load(f))
    out = {}
    for name in names:
        g = np.load(os.path.join(GOLDEN, "post_%s.npz" % name))
        out[name] = (np.asarray(g["val_entries"], dtype=np.float64).reshape(-1, 20), np.asarray(g["val_allk"], dtype=np.float64).reshape(-1, 4))
    return out


def _kpts(n, seed):
    r = np.random.RandomState(seed)
    k = np.zeros((n, 4), dtype=np.float64)
    k[:, 0] = r.randint(0, 640, size=n)
    k[:, 1] = r.randint(0, 480, size=n)
    k[:, 2] = r.uniform(0.1, 1.0, size=n).astype(np.float32)
    k[:, 3] = np.arange(n)
    return k


def _entry(ids, score, count):
    row = np.full(20, -1.0)
    for t, i in ids.items():
        row[t] = float(i)
    row[18], row[19] = score, count
    return row


def _poses(n, nk, seed):
    """n poses over nk key-points with a random subset of the 18 types each."""
    r = np.random.RandomState(seed)
    rows = []
    for _ in range(n):
        types = r.choice(18, size=r.randint(3, 19), replace=False)
        rows.append(_entry({int(t): int(r.randint(0, nk)) for t in types}, float(r.uniform(1.0, 30.0)), float(len(types))))
    return np.array(rows).reshape(-1, 20)


def edge_batches(max_entries=256):
    """name -> list of frames (one call of the append kernel each), the issue's edge inputs."""
    k40 = _kpts(40, 3)
    return {
        # the prefix over the frames of a call, and a frame without a pose in the middle
        "batch_2_0_5": [(_poses(2, 40, 1), k40), (np.zeros((0, 20)), np.zeros((0, 4))), (_poses(5, 40, 2), k40)],
        # a frame at the workspace's pose capacity: more poses than the workgroup has threads would be 257; 256 is the limit
        "full_frame": [(_poses(max_entries, 300, 4), _kpts(300, 5))],
        "one_keypoint_left": [(np.array([_entry({9: 7}, 3.5, 3.0)]), k40)],
        # count 1: the score is x * 0 = 0.0 (and -0.0 for a negative x, as NumPy gives it)
        "count_one": [(np.array([_entry({4: 2}, 2.25, 1.0), _entry({4: 3}, -2.25, 1.0), _entry({4: 3}, 2.0, 0.0)]), k40)],
        # the neck alone: every slot stays (0, 0, 0)
        "neck_only": [(np.array([_entry({1: 11}, 4.0, 3.0)]), k40)],
    }
