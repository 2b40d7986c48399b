"""Device-side pose tail on the GPU (-m gpu): un-map, Pose rows, tracking and 1-Euro smoothing behind the grouping kernels.
Every comparison is exact: ids, int32 key-points, boxes, counts, the id counter.  The references are the reference
implementation's own outputs (tests/golden/tail_*.npz, tracking.json) and, end to end, the Python tail
(demo.poses_from_entries + modules.pose.track_poses, tied to the same fixtures by tests/test_tracking_host.py) applied to the
entries of the same call.  Every fixture test also asserts that no similarity decision lay within 1e-12 of the threshold."""
import ctypes as C

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo, synth, workload
from lwpose_amd.modules import pose as pose_mod
from lwpose_amd.runtime import Engine

import skeleton_cases as sc
import tracking_cases as tc

pytestmark = pytest.mark.gpu

SKIPPED_JSON = ("no_ids_seed10", "no_ids_thr0_seed11")     # previous poses without ids: a state the device tracker cannot be in


def replay(eng, frames, K, lane=0):
    """frames: [(in_kp, in_conf, out_kp, out_bbox, out_ids, last_id)] through lwp_track_poses; returns (inherited, fresh after
    frame 0, coordinates moved)."""
    prev_ids, inherited, fresh, moved, last = set(), 0, 0, 0, -1
    for t, (ikp, icf, okp, obb, oid, lid) in enumerate(frames):
        r = eng.track_poses_device(np.asarray(ikp, np.int32).reshape(-1, K, 2), icf, lane)
        assert r["near"] == 0, t
        assert np.array_equal(r["ids"], np.asarray(oid, np.int32).reshape(-1)), t
        assert np.array_equal(r["keypoints"], np.asarray(okp, np.int32).reshape(-1, K, 2)), t
        assert np.array_equal(r["bbox"], np.asarray(obb, np.int32).reshape(-1, 4)), t
        assert r["last_id"] == lid, t
        inherited += sum(1 for i in r["ids"].tolist() if i in prev_ids)
        fresh += (lid - last) if t > 0 else 0
        moved += int((r["keypoints"] != np.asarray(ikp, np.int32).reshape(-1, K, 2)).sum())
        prev_ids, last = set(r["ids"].tolist()), lid
    return inherited, fresh, moved


def test_tracking_json_cases_through_track_poses():
    eng = Engine(0)
    names = []
    for case in tc.json_cases():
        if case["name"] in SKIPPED_JSON:
            continue
        names.append(case["name"])
        eng.set_tracking(Engine.TRACK_LANES, match_threshold=case["threshold"], smooth=case["smooth"])
        frames = [(f["in_keypoints"], f["in_confidence"], f["keypoints"], f["bbox"], f["ids"], f["last_id"]) for f in case["frames"]]
        replay(eng, frames, 18)
    assert len(names) == len(tc.json_cases()) - 2 >= 17


@pytest.mark.parametrize("name", tc.tracking_case_names())
def test_tracking_fixture_through_track_poses(name):
    c = tc.tracking_case(name)
    K = c["K"]
    if K == 18:
        eng = Engine(0)
    else:
        kpts, pafs = (sc.GUIDE5_KPTS, sc.GUIDE5_PAFS) if K == 5 else (sc.HAND21_KPTS, sc.HAND21_PAFS)
        eng = Engine(0, num_heatmaps=K + 1, num_pafs=2 * len(kpts))
        eng.set_skeleton(kpts, pafs, K, max(20, K + 2))
    eng.set_tracking(Engine.TRACK_SEQUENCE, c["match_threshold"], c["similarity_threshold"], c["smooth"], sigmas=c["sigmas"])
    frames = [(f["in_kp"], f["in_conf"], f["out_kp"], f["out_bbox"], f["out_ids"], f["last_id"]) for f in c["frames"]]
    inherited, fresh, moved = replay(eng, frames, K)
    assert (inherited > 0) == (c["match_threshold"] <= K) and fresh > 0
    assert (moved > 0) == (c["smooth"] and c["match_threshold"] <= K)
    if name.startswith("crowd150"):
        assert max(len(f[0]) for f in frames) > 128          # more poses than two waves have lanes


@pytest.mark.parametrize("name", tc.unmap_case_names())
def test_unmap_fixture_through_poses_from_maps(name):
    c = tc.unmap_case(name)
    heat, paf, _ = synth.make_pose_maps(*c["maps"])
    eng = Engine(0)
    eng.set_tracking(Engine.TRACK_ROWS)
    eng.set_unmap(c["stride"], c["scale"], c["pad"])
    ent, allk, _ = eng.poses_from_maps(heat[None], paf[None], c["ratio"], True)[0]
    assert np.array_equal(ent, c["entries"]) and np.array_equal(allk, c["all_keypoints"])
    rows = eng.poses()[0]
    assert np.array_equal(rows["keypoints"], c["out_kp"])
    assert np.array_equal(rows["confidence"], c["out_conf"])
    assert np.array_equal(rows["bbox"], c["out_bbox"])
    assert (rows["ids"] == -1).all() and rows["last_id"] == -1


# ------------------------------------------------------------------------------------------ end to end on moving maps
def moving_maps(make, n_frames=9):
    """People that drift one low-resolution pixel per frame (wrapping at the border); from frame 5 on another crowd."""
    out = []
    for t in range(n_frames):
        heat, paf = make(0 if t < 5 else 1)
        out.append((np.roll(heat, t, axis=2).copy(), np.roll(paf, t, axis=2).copy()))
    return out


def python_tail(monkeypatch, K, sigmas, results, geometry, smooth, match_threshold=3):
    """The Python tail on the entries of the device calls: [(kp (P,K,2), bbox (P,4), ids (P,), last_id)] per frame."""
    stride, scale, pad, ratio = geometry
    monkeypatch.setattr(pose_mod.Pose, "num_kpts", K)
    monkeypatch.setattr(pose_mod.Pose, "sigmas", sigmas)
    monkeypatch.setattr(pose_mod.Pose, "vars", (sigmas * 2) ** 2)
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    prev, out = [], []
    for ent, allk in results:
        assert ent.shape[1] == 20                    # poses_from_entries reads the score at the reference's literal column 18 = E - 2
        cur = demo.poses_from_entries(ent, allk, scale, pad, stride, ratio)
        pose_mod.track_poses(prev, cur, threshold=match_threshold, smooth=smooth)
        out.append((np.stack([p.keypoints for p in cur]).reshape(-1, K, 2), np.array([p.bbox for p in cur], np.int32).reshape(-1, 4),
                    np.array([p.id for p in cur], np.int32), pose_mod.Pose.last_id))
        prev = cur
    return out


def run_moving(monkeypatch, eng, K, sigmas, frames, ratio, smooth, mode=Engine.TRACK_LANES, batch=1):
    geometry = (8, 0.731, [3, 5, 0, 0], ratio)
    eng.set_tracking(mode, smooth=smooth, sigmas=sigmas)
    eng.set_unmap(8, 0.731, [3, 5, 0, 0])
    results, device = [], []
    for b in range(0, len(frames), batch):
        heat = np.stack([f[0] for f in frames[b:b + batch]])
        paf = np.stack([f[1] for f in frames[b:b + batch]])
        res = eng.poses_from_maps(heat, paf, ratio, True)
        rows = eng.poses()
        for (ent, allk, _), r in zip(res, rows):
            assert r["near"] == 0
            results.append((ent, allk))
            device.append((r["keypoints"], r["bbox"], r["ids"], r["last_id"]))
    want = python_tail(monkeypatch, K, sigmas, results, geometry, smooth)
    inherited = fresh = 0
    for t, (d, w) in enumerate(zip(device, want)):
        for a, b in zip(d[:3], w[:3]):
            assert np.array_equal(a, b), t
        assert d[3] == w[3], t
        if t > 0:
            inherited += len(set(d[2].tolist()) & set(device[t - 1][2].tolist()))
            fresh += d[3] - device[t - 1][3]
    assert inherited > 0 and fresh > 0                # an empty comparison cannot pass
    return device


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("smooth", [False, True])
def test_moving_coco_maps_equal_python_tail(monkeypatch, generic, smooth):
    if generic:
        monkeypatch.setenv("LWP_POST_GENERIC", "1")
    eng = Engine(0)
    assert bool(eng.post_generic) == generic
    frames = moving_maps(lambda s: synth.make_pose_maps(5 + 2 * s, 46, 82, 4 + s, 0.1, 0.01)[:2])
    dev = run_moving(monkeypatch, eng, 18, pose_mod._SIGMAS.copy(), frames, 4, smooth)
    if smooth:
        plain = run_moving(monkeypatch, eng, 18, pose_mod._SIGMAS.copy(), frames, 4, False)
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(dev, plain))      # smoothing moved a coordinate


@pytest.mark.parametrize("smooth", [False, True])
def test_moving_custom_skeleton_maps_equal_python_tail(monkeypatch, smooth):
    case = sc.map_case("guide5_r4")
    _, canon, kpts, pafs, npafs, n, h, w, seed, drop, noise, ratio = case
    eng = Engine(0, num_heatmaps=6, num_pafs=npafs)
    eng.set_skeleton(kpts, pafs, 5, 20)
    sig = (np.array([.5, .9, .8, .8, .3], dtype=np.float32) / 10.0)
    frames = moving_maps(lambda s: synth.make_skeleton_maps(canon, kpts, pafs, npafs, n + s, h, w, seed + s, drop, noise)[:2])
    dev = run_moving(monkeypatch, eng, 5, sig, frames, ratio, smooth)
    if smooth:
        plain = run_moving(monkeypatch, eng, 5, sig, frames, ratio, False)
        assert any(not np.array_equal(a[0], b[0]) for a, b in zip(dev, plain))


def coco_frames(n=8):
    return moving_maps(lambda s: synth.make_pose_maps(5 + 2 * s, 46, 82, 4 + s, 0.1, 0.01)[:2], n)


def rows_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_lanes_interleaved_equal_single_lane_runs(monkeypatch):
    frames = coco_frames(8)
    # lane l sees the sequence shifted by l frames
    seqs = [[frames[(t + l) % 8] for t in range(6)] for l in range(4)]
    eng = Engine(0)
    eng.set_tracking(Engine.TRACK_LANES, smooth=True)
    multi = [[] for _ in range(4)]
    for t in range(6):
        eng.poses_from_maps(np.stack([seqs[l][t][0] for l in range(4)]), np.stack([seqs[l][t][1] for l in range(4)]), 4, True)
        for l, r in enumerate(eng.poses()):
            multi[l].append((r["keypoints"], r["bbox"], r["ids"], r["last_id"]))
    for l in range(4):
        single = Engine(0)
        single.set_tracking(Engine.TRACK_LANES, smooth=True)
        for t in range(6):
            single.poses_from_maps(seqs[l][t][0][None], seqs[l][t][1][None], 4, True)
            r = single.poses()[0]
            assert rows_equal(multi[l][t], (r["keypoints"], r["bbox"], r["ids"], r["last_id"])), (l, t)
    assert multi[0][5][3] > multi[0][0][3] >= 0


def test_reset_with_next_id_and_lane_independence():
    frames = coco_frames(3)
    eng = Engine(0)
    eng.set_tracking(Engine.TRACK_LANES)
    eng.reset_tracking(1, 100)
    eng.poses_from_maps(np.stack([frames[0][0]] * 2), np.stack([frames[0][1]] * 2), 4, True)
    a, b = eng.poses()
    n = len(a["ids"])
    assert n >= 2 and sorted(a["ids"].tolist()) == list(range(n)) and a["last_id"] == n - 1
    assert sorted(b["ids"].tolist()) == list(range(100, 100 + n)) and b["last_id"] == 99 + n
    eng.reset_tracking(-1, 7)
    eng.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)
    assert sorted(eng.poses()[0]["ids"].tolist()) == list(range(7, 7 + n))


# ------------------------------------------------------------------------------------------ the network path
@pytest.fixture(scope="module")
def net368():
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    return net


def net_frames(n):
    fr = synth.make_frames(1, 368, 656, seed0=0)[0]
    # the calibrated workload, drifting: frame t is frame 0 moved by 8 pixels (one cell of the stride-8 maps) per step
    x = np.stack([np.roll(fr, 8 * t, axis=1) for t in range(n)])
    return torch.from_numpy(workload.normalized_input(x)).cuda()


def tail_rows(r):
    return (r["keypoints"], r["bbox"], r["ids"], r["last_id"])


def test_network_path_equals_python_tail(monkeypatch, net368):
    eng = net368.engine
    x = net_frames(8)
    geometry = (8, 368 / 720, [0, 2, 0, 0], 4)
    eng.set_tracking(Engine.TRACK_LANES, smooth=True)
    try:
        eng.set_unmap(8, 368 / 720, [0, 2, 0, 0])
        results, device = [], []
        for t in range(8):
            ent, allk, _ = eng.infer_poses(x[t:t + 1], 4, True)[0]
            r = eng.poses()[0]
            assert r["near"] == 0
            results.append((ent, allk))
            device.append(tail_rows(r))
        want = python_tail(monkeypatch, 18, pose_mod._SIGMAS.copy(), results, geometry, True)
        for t in range(8):
            assert rows_equal(device[t], want[t]), t
        inherited = sum(len(set(device[t][2].tolist()) & set(device[t - 1][2].tolist())) for t in range(1, 8))
        assert len(device[0][2]) >= 10 and inherited > 0 and device[7][3] > device[0][3]
    finally:
        eng.set_tracking(Engine.TRACK_OFF)


def test_sequence_batch_equals_batch1_calls_and_split(monkeypatch, net368):
    eng = net368.engine
    x = net_frames(8)
    try:
        eng.set_tracking(Engine.TRACK_SEQUENCE, smooth=True)
        eng.set_unmap(8, 0.5, [1, 2, 0, 0])          # the geometry is handle state: both engines of this test get the same
        one = []
        for t in range(8):
            eng.infer_poses(x[t:t + 1], 4, True)
            one.append(tail_rows(eng.poses()[0]))
        eng.set_tracking(Engine.TRACK_SEQUENCE, smooth=True)
        eng.infer_poses(x, 4, True)
        batch = [tail_rows(r) for r in eng.poses()]
        for t in range(8):
            assert rows_equal(one[t], batch[t]), t
        inherited = sum(len(set(one[t][2].tolist()) & set(one[t - 1][2].tolist())) for t in range(1, 8))
        assert inherited > 0 and one[7][3] > one[0][3]
    finally:
        eng.set_tracking(Engine.TRACK_OFF)
    monkeypatch.setenv("LWP_MAX_FRAMES_PER_PASS", "3")
    net2, _ = workload.build_net(nref=1, seed=1, device=0)
    e2 = net2.engine
    assert e2.frames_per_pass(8, 368, 656) == 3
    e2.set_tracking(Engine.TRACK_SEQUENCE, smooth=True)
    e2.set_unmap(8, 0.5, [1, 2, 0, 0])
    e2.infer_poses(x, 4, True)
    for t, r in enumerate(e2.poses()):
        assert rows_equal(one[t], tail_rows(r)), t


def test_pipeline_slots_equal_serial(net368):
    eng = net368.engine
    x = net_frames(6)
    try:
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        serial = []
        for t in range(6):
            eng.infer_poses(x[t:t + 1], 4, True)
            serial.append(tail_rows(eng.poses()[0]))
        eng.set_tracking(Engine.TRACK_LANES, smooth=True)
        eng.pipeline_submit(x[0:1].contiguous(), 0)
        with pytest.raises(RuntimeError, match="pending"):
            eng.set_tracking(Engine.TRACK_OFF)                       # refused while a slot is pending
        got = []
        for t in range(1, 6):
            eng.pipeline_submit(x[t:t + 1].contiguous(), t % 2)      # submit(k + 1) before fetch(k)
            with pytest.raises(RuntimeError, match="pending"):
                eng.poses((t - 1) % 2)
            eng.pipeline_fetch((t - 1) % 2)
            got.append(tail_rows(eng.poses((t - 1) % 2)[0]))
        eng.pipeline_fetch(5 % 2)
        got.append(tail_rows(eng.poses(5 % 2)[0]))
        for t in range(6):
            assert rows_equal(serial[t], got[t]), t
    finally:
        eng.synchronize()
        eng.set_tracking(Engine.TRACK_OFF)


# ------------------------------------------------------------------------------------------ state, errors, tail off
def test_state_and_errors():
    frames = coco_frames(2)
    eng = Engine(0)
    eng.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)
    with pytest.raises(RuntimeError, match="pose tail was off"):
        eng.poses()
    with pytest.raises(RuntimeError, match="tracking is off"):
        eng.track_poses_device(np.zeros((1, 18, 2), np.int32), [1.0])
    with pytest.raises(RuntimeError, match="tracking is off"):
        eng.reset_tracking(0, 0)
    eng.set_tracking(Engine.TRACK_LANES)
    ent, _, _ = eng.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)[0]
    n = len(ent)
    assert n >= 2
    ip = C.POINTER(C.c_int)
    bufs = [np.zeros(4096, np.int32) for _ in range(5)]
    conf = np.zeros(64, np.float64)
    rc = _lib.lib().lwp_get_poses(eng.h.ptr, -1, bufs[0].ctypes.data_as(ip), bufs[1].ctypes.data_as(ip),
                                  conf.ctypes.data_as(C.POINTER(C.c_double)), bufs[2].ctypes.data_as(ip), bufs[3].ctypes.data_as(ip),
                                  None, n - 1)
    assert rc == _lib.LWP_ERR_CAPACITY and b"pose_cap" in _lib.lib().lwp_last_error(eng.h.ptr)
    first = eng.poses()[0]
    assert sorted(first["ids"].tolist()) == list(range(n))
    eng.poses_from_maps(frames[1][0][None], frames[1][1][None], 4, True)
    assert len(set(eng.poses()[0]["ids"].tolist()) & set(first["ids"].tolist())) > 0          # ids carried over
    # a custom sigma count is checked against the skeleton's K on a real handle
    with pytest.raises(ValueError, match="n_sigmas is 5"):
        eng.set_tracking(Engine.TRACK_LANES, sigmas=[0.05] * 5)
    # lwp_set_skeleton clears the lanes (same K: tracking stays on, ids start over)
    eng.set_skeleton(sc.COCO_KPTS, sc.COCO_PAFS, 18, 20)
    eng.poses_from_maps(frames[1][0][None], frames[1][1][None], 4, True)
    again = eng.poses()[0]
    assert sorted(again["ids"].tolist()) == list(range(len(again["ids"])))
    # another K: NULL sigmas are refused, and tracking went off with the old table
    e5 = Engine(0, num_heatmaps=6, num_pafs=8)
    e5.set_tracking(Engine.TRACK_LANES)
    e5.set_skeleton(sc.GUIDE5_KPTS, sc.GUIDE5_PAFS, 5, 20)
    with pytest.raises(RuntimeError, match="tracking is off"):
        e5.reset_tracking(0, 0)
    with pytest.raises(ValueError, match="sigmas is NULL"):
        e5.set_tracking(Engine.TRACK_LANES)
    # more than 256 pose slots per frame: refused while the tail is on
    big = Engine(0)
    big.set_capacity(max_entries=300)
    big.set_tracking(Engine.TRACK_ROWS)
    with pytest.raises(ValueError, match="256 poses"):
        big.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)


def test_tail_off_is_identical_to_an_untouched_handle(net368):
    x = net_frames(2)
    net2, _ = workload.build_net(nref=1, seed=1, device=0)
    fresh, eng = net2.engine, net368.engine
    eng.set_tracking(Engine.TRACK_LANES, smooth=True)
    eng.infer_poses(x, 4, True)
    on = eng.profile_launches(x[:1].contiguous(), reps=1)
    eng.set_tracking(Engine.TRACK_OFF)
    a = eng.infer_poses(x, 4, True)
    b = fresh.infer_poses(x, 4, True)
    for (e1, k1, c1), (e2, k2, c2) in zip(a, b):
        assert np.array_equal(e1, e2) and np.array_equal(k1, k2) and np.array_equal(c1, c2)
    pa = eng.profile_launches(x[:1].contiguous(), reps=1)
    pb = fresh.profile_launches(x[:1].contiguous(), reps=1)
    assert [(n, k) for n, k, _ in pa] == [(n, k) for n, k, _ in pb]
    assert len(on) == len(pa) + 2 and [n for n, _, _ in on[-2:]] == ["tail_rows", "tail_track"]     # the tail is two launches
    n_layers = len(eng.layers())
    assert [eng.layer_variant(i) for i in range(n_layers)] == [fresh.layer_variant(i) for i in range(n_layers)]
    with pytest.raises(RuntimeError, match="pose tail was off"):
        eng.poses()


def test_run_demo_device_tail_equals_python_tail(net368):
    frames = [np.ascontiguousarray(f) for f in synth.make_frames(4, 720, 1280, seed0=0)]
    frames = frames + [np.roll(f, 16, axis=1).copy() for f in frames]
    pose_mod.Pose.last_id = -1
    want = [(np.stack([p.keypoints for p in poses]), [p.bbox for p in poses], [p.id for p in poses])
            for _, poses in demo.run_demo(net368, [f.copy() for f in frames], 368, False, True, True, fused=True)]
    last_python = pose_mod.Pose.last_id
    pose_mod.Pose.last_id = -1
    got = [(np.stack([p.keypoints for p in poses]), [p.bbox for p in poses], [p.id for p in poses])
           for _, poses in demo.run_demo(net368, [f.copy() for f in frames], 368, False, True, True, fused=True, device_tail=True)]
    assert pose_mod.Pose.last_id == last_python >= 0
    for t, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(w[0], g[0]) and w[1] == g[1] and w[2] == g[2], t
    pose_mod.Pose.last_id = -1


# ------------------------------------------------------------------------------------------ limits: 256 poses, 64 types, bad scores
def synthetic_crowd(seed, n_frames, n_people, K):
    """Seeded drifting crowd, n_people poses in every frame (input order reshuffled), some key-points missing, shared scores."""
    rng = np.random.RandomState(seed)
    cols = int(np.ceil(np.sqrt(n_people)))
    origin = np.stack([(np.arange(n_people) % cols) * 80 + 50, (np.arange(n_people) // cols) * 80 + 50], 1)[:, None, :]
    shape = rng.randint(-25, 26, size=(n_people, K, 2))
    vel = rng.randint(-4, 5, size=(n_people, 1, 2))
    conf = np.round(rng.rand(n_people) * 10, 2)
    frames = []
    for t in range(n_frames):
        order = rng.permutation(n_people)
        kp = (origin + shape + vel * t + rng.randint(-2, 3, size=(n_people, K, 2))).astype(np.int32)
        kp[rng.rand(n_people, K) < 0.1] = -1
        if t == 2:
            kp[::7] = np.where(kp[::7] != -1, kp[::7] + 20000, -1)      # every seventh pose jumps away: fresh ids
        frames.append((kp[order], conf[order]))
    return frames


def replay_against_python_tail(monkeypatch, eng, frames, K, sigmas, smooth):
    monkeypatch.setattr(pose_mod.Pose, "num_kpts", K)
    monkeypatch.setattr(pose_mod.Pose, "sigmas", sigmas)
    monkeypatch.setattr(pose_mod.Pose, "vars", (sigmas * 2) ** 2)
    monkeypatch.setattr(pose_mod.Pose, "last_id", -1)
    eng.set_tracking(Engine.TRACK_LANES, smooth=smooth, sigmas=sigmas)
    prev, want = [], []
    for kp, cf in frames:
        cur = [pose_mod.Pose(k.copy(), float(c)) for k, c in zip(kp, cf)]
        pose_mod.track_poses(prev, cur, smooth=smooth)
        want.append((kp, cf, np.stack([p.keypoints for p in cur]), [p.bbox for p in cur], [p.id for p in cur], pose_mod.Pose.last_id))
        prev = cur
    return replay(eng, want, K)


def test_256_poses_per_frame_equal_python_tail(monkeypatch):
    """P = 256 exactly: all four register slots of the greedy pass (previous poses 192..255 included)."""
    frames = synthetic_crowd(7, 4, 256, 18)
    eng = Engine(0)
    assert eng.caps[3] == 256
    inherited, fresh, moved = replay_against_python_tail(monkeypatch, eng, frames, 18, pose_mod._SIGMAS.copy(), True)
    assert inherited > 500 and fresh >= 30 and moved > 0      # ~219 of 256 carry their id in each later frame
    with pytest.raises(_lib.CapacityError, match="max_pose_entries"):
        eng.track_poses_device(np.zeros((257, 18, 2), np.int32), np.ones(257))


def test_64_keypoint_types_equal_python_tail(monkeypatch):
    K = 64
    kpts = [[i, i + 1] for i in range(K - 1)]
    pafs = [[2 * i, 2 * i + 1] for i in range(K - 1)]
    eng = Engine(0, num_heatmaps=K + 1, num_pafs=2 * (K - 1))
    eng.set_skeleton(kpts, pafs, K, K + 2)
    sig = (np.linspace(0.25, 1.07, K).astype(np.float32) / np.float32(10.0)).astype(np.float32)
    frames = synthetic_crowd(9, 4, 40, K)
    inherited, fresh, moved = replay_against_python_tail(monkeypatch, eng, frames, K, sig, True)
    assert inherited > 60 and fresh > 0 and moved > 0


def test_non_finite_confidence_is_refused():
    eng = Engine(0)
    eng.set_tracking(Engine.TRACK_LANES)
    kp = np.full((3, 18, 2), 10, np.int32)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            eng.track_poses_device(kp, [1.0, bad, 2.0])
    r = eng.track_poses_device(kp, [1.0, 3.0, 2.0])                     # the lane is untouched by the refused calls
    assert r["ids"].tolist() == [2, 0, 1] and r["last_id"] == 2


def test_other_users_of_the_workspace_drop_the_pose_rows(net368):
    frames = coco_frames(1)
    eng = Engine(0)
    eng.set_tracking(Engine.TRACK_LANES)
    ent, allk, counts = eng.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)[0]
    assert len(eng.poses()[0]["ids"]) == len(ent) >= 2
    # lwp_group_keypoints has no tail: nothing to return afterwards (not the rows of the earlier call)
    pu = np.ascontiguousarray(np.zeros((184, 328, 38), np.float32))
    eng.group_keypoints(allk, counts, pu, True)
    with pytest.raises(RuntimeError, match="no pose rows"):
        eng.poses()
    eng.poses_from_maps(frames[0][0][None], frames[0][1][None], 4, True)
    eng.extract_keypoints(np.zeros((64, 64), np.float32))               # reuses the pinned staging block
    with pytest.raises(RuntimeError, match="no pose rows"):
        eng.poses()
    # lwp_track_poses takes frame 0 of the serial workspace: an unfetched async run is gone, and so are its rows
    e = net368.engine
    x = net_frames(1)
    try:
        e.set_tracking(Engine.TRACK_LANES)
        e.infer_poses_async(x)
        e.track_poses_device(np.full((1, 18, 2), 10, np.int32), [1.0])
        with pytest.raises(RuntimeError, match="no pipeline run to fetch"):
            e.fetch_poses()
        with pytest.raises(RuntimeError, match="no pose rows"):
            e.poses()
        # the lanes belong to one stream at a time: no serial pass while a slot is pending
        e.pipeline_submit(x, 0)
        with pytest.raises(RuntimeError, match="pipeline slot is pending"):
            e.infer_poses(x, 4, True)
        e.pipeline_fetch(0)
        e.infer_poses(x, 4, True)
        assert len(e.poses()[0]["ids"]) >= 10
    finally:
        e.synchronize()
        e.set_tracking(Engine.TRACK_OFF)
