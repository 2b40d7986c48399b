"""Shared by tests/test_video_host.py (CPU) and tests/test_gpu_video.py: the frames and geometries of the one-call video step and
their expected values from the oracle (oracle/preproc_ref.py, net_ref.py, post_ref.py, tail_ref.py — imported, not restated).

The weights are the seeded random-init state dict of the benchmark workload with the last head layer calibrated from the
ORACLE network's maps of frame 0 (synth.calibrate_heads takes the maps of any forward provider), so the CPU test and the GPU test
talk about the same network without a GPU being needed to build it."""
import functools

import numpy as np
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth, workload
from oracle import net_ref, post_ref, preproc_ref, tail_ref

# (H, W, net_input_height, stride): both need a resize (scale != 1) and a left pad (pad != 0)
PIPE_GEOMETRIES = {"720x1280": (720, 1280, 368, 8), "480x640": (480, 640, 368, 8)}


@functools.lru_cache(maxsize=None)
def state_dict():
    sd = synth.make_state_dict(1, seed=1)
    frame0 = synth.make_frames(1, 368, 656, seed0=0)
    outs = net_ref.forward(sd, torch.from_numpy(workload.normalized_input(frame0)), 1)
    return synth.calibrate_heads(sd, outs[-2][0].numpy(), outs[-1][0].numpy(), 1)


def pipe_frames(name, n, seed0=0):
    H, W, _, _ = PIPE_GEOMETRIES[name]
    return [np.ascontiguousarray(f) for f in synth.make_frames(n, H, W, seed0=seed0)]


def oracle_post(heat_chw, paf_chw, ratio=4):
    """post_ref on stride-8 maps: (entries (P,20) f64, all_keypoints (n,4) f64)."""
    hu = post_ref.upsample_cubic(np.ascontiguousarray(heat_chw.transpose(1, 2, 0)), ratio)
    pu = post_ref.upsample_cubic(np.ascontiguousarray(paf_chw.transpose(1, 2, 0)), ratio)
    by_type, total = [], 0
    for k in range(18):
        total += post_ref.extract_keypoints(hu[:, :, k], by_type, total)
    ent, allk = post_ref.group_keypoints(by_type, pu, demo=True)
    return np.asarray(ent, dtype=np.float64).reshape(-1, 20), np.asarray(allk, dtype=np.float64).reshape(-1, 4)


def oracle_maps(frame, name):
    """preproc_ref -> net_ref: (x (1,3,H',W') f32, heat (19,h,w), paf (38,h,w), scale, pad)."""
    _, _, net_h, stride = PIPE_GEOMETRIES[name]
    x, scale, pad = preproc_ref.prepare_frame(frame, net_h, stride)
    outs = net_ref.forward(state_dict(), torch.from_numpy(x), 1)
    return x, outs[-2][0].numpy(), outs[-1][0].numpy(), scale, pad


def oracle_chain(frame, name):
    """preproc_ref -> net_ref -> post_ref: (entries, all_keypoints, scale, pad)."""
    _, heat, paf, scale, pad = oracle_maps(frame, name)
    ent, allk = oracle_post(heat, paf)
    return ent, allk, scale, pad


class OracleTail(object):
    """tail_ref over a sequence of frames of one lane: poses_from_entries + track_poses with the reference's own state (the
    previous poses with their filters, the id counter)."""

    def __init__(self, track, smooth, first_id=0):
        self.track, self.smooth, self.prev, self.last_id = track, smooth, [], first_id - 1

    def step(self, ent, allk, scale, pad, stride=8, ratio=4):
        """-> (keypoints (P,18,2) int32, bbox (P,4) int32, ids (P,) int32, confidence (P,), last_id)"""
        cur = tail_ref.poses_from_entries(ent, allk.copy(), scale, pad, stride, ratio)
        conf = np.array([p.confidence for p in cur], np.float64)
        if self.track:
            tail_ref.RefPose.last_id = self.last_id
            tail_ref.track_poses(self.prev, cur, smooth=self.smooth)
            self.last_id = tail_ref.RefPose.last_id
            self.prev = cur
        kp = np.stack([p.keypoints for p in cur]).reshape(-1, 18, 2).astype(np.int32) if cur else np.zeros((0, 18, 2), np.int32)
        bbox = np.array([p.bbox for p in cur], np.int32).reshape(-1, 4)
        ids = np.array([p.id if self.track else -1 for p in cur], np.int32)
        return kp, bbox, ids, conf, (self.last_id if self.track else -1)
