"""Readers of the pose-tail fixtures (tests/golden/tail_*.npz, tools/make_tracking_golden.py) and of tracking.json, shared by
the host and the GPU tracking tests.  Inputs are stored with the reference's outputs; nothing is regenerated here except the
synthetic maps of the un-map cases (from the stored generator parameters)."""
import json
import os

import numpy as np

from conftest import GOLDEN

TRACK_FILES = ("crowd35", "crowd70", "crowd150", "thresholds", "skeletons")


def tracking_case_names():
    out = []
    for f in TRACK_FILES:
        g = np.load(os.path.join(GOLDEN, "tail_%s.npz" % f))
        out += ["%s/%s" % (f, c) for c in g["cases"].tolist()]
    return out


def tracking_case(name):
    """dict(K, match_threshold, smooth, similarity_threshold, sigmas, frames=[dict(in_kp, in_conf, out_kp, out_bbox, out_ids, last_id)])"""
    f, c = name.split("/")
    g = np.load(os.path.join(GOLDEN, "tail_%s.npz" % f))
    K, thr, smooth, nf = [int(v) for v in g[c + ":meta"]]
    n = g[c + ":n"]
    off = np.concatenate([[0], np.cumsum(n)])
    frames = []
    for t in range(nf):
        s = slice(off[t], off[t + 1])
        frames.append(dict(in_kp=g[c + ":in_kp"][s], in_conf=g[c + ":in_conf"][s], out_kp=g[c + ":out_kp"][s],
                           out_bbox=g[c + ":out_bbox"][s], out_ids=g[c + ":out_ids"][s], last_id=int(g[c + ":last_id"][t])))
    return dict(K=K, match_threshold=thr, smooth=bool(smooth), similarity_threshold=float(g[c + ":similarity_threshold"]),
                sigmas=g[c + ":sigmas"], frames=frames)


def unmap_case_names():
    return np.load(os.path.join(GOLDEN, "tail_unmap.npz"))["cases"].tolist()


def unmap_case(name):
    g = np.load(os.path.join(GOLDEN, "tail_unmap.npz"))
    ratio, stride, pad_top, pad_left = [int(v) for v in g[name + ":geometry"]]
    mp = g[name + ":maps"]
    maps = (int(mp[0]), int(mp[1]), int(mp[2]), int(mp[3]), float(mp[4]), float(mp[5]))
    return dict(maps=maps, ratio=ratio, stride=stride, pad=[pad_top, pad_left, 0, 0], scale=float(g[name + ":scale"]),
                entries=g[name + ":entries"], all_keypoints=g[name + ":all_keypoints"], out_kp=g[name + ":out_kp"],
                out_conf=g[name + ":out_conf"], out_bbox=g[name + ":out_bbox"])


def json_cases():
    """The sequences of tests/golden/tracking.json (oracle/make_golden.py gen_tracking)."""
    with open(os.path.join(GOLDEN, "tracking.json")) as f:
        return json.load(f)["cases"]
