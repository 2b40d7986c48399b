"""Generates tests/golden/tail_*.npz: the reference's own pose tail (demo.py:101-114 un-map + Pose rows, modules/pose.py
get_similarity / track_poses with its 1-Euro smoothing) on seeded crowds and on grouped synthetic maps.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_tracking_golden.py

The reference's statements are executed, not restated: ``Pose`` / ``get_similarity`` / ``track_poses`` come from
``oracle.make_golden.ref_pose_namespace`` (parsed out of modules/pose.py, bounding-box stand-in as documented there), the two
loops of demo.py:101-114 are parsed out of ``run_demo``.  ``get_similarity``'s threshold is a default argument that
``track_poses`` never passes, so other similarity thresholds are set on the parsed function's ``__defaults__``.  Inputs are
stored with the outputs.  Every case asserts what it is for, and the smallest |exp(-q) - threshold| met is printed: the device
decides q < -ln(threshold) instead, which can differ only within a few ulp of the threshold.
"""
import ast
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("LWP_REFERENCE", "/root/reference")

import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth  # noqa: E402
from oracle import post_ref  # noqa: E402
from oracle.make_golden import ref_pose_namespace  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def save(name, d):
    path = os.path.join(OUT, "tail_%s.npz" % name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:       # fixed dates: two runs give identical files
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 900 * 1024, (path, os.path.getsize(path))
    print("%8d  %s" % (os.path.getsize(path), os.path.basename(path)))


class NpSpy(object):
    """numpy with an ``exp`` that records how close a similarity came to the threshold."""

    def __init__(self):
        self.threshold = 0.5
        self.closest = np.inf

    def __getattr__(self, name):
        return getattr(np, name)

    def exp(self, v):
        r = np.exp(v)
        self.closest = min(self.closest, float(abs(r - self.threshold)))
        return r


def demo_tail_loops():
    """The statements of demo.py:101-114 (un-map loop, ``current_poses = []``, the Pose loop) of the reference's run_demo."""
    tree = ast.parse(open(os.path.join(REF, "demo.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run_demo"][0]
    loop = [n for n in fn.body if isinstance(n, ast.For) and getattr(n.target, "id", "") == "img"][0]
    keep = []
    for n in loop.body:
        if isinstance(n, ast.For) and getattr(n.target, "id", "") in ("kpt_id", "n"):
            keep.append(n)
        elif isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "current_poses":
            keep.append(n)
    assert [type(n).__name__ for n in keep] == ["For", "Assign", "For"], keep
    mod = ast.Module(keep, [])
    ast.fix_missing_locations(mod)
    return compile(mod, os.path.join(REF, "demo.py"), "exec")


# ------------------------------------------------------------------------------------------------ crowds
def crowd(seed, n_frames, n_people, K, equal_conf=True, strangers=False):
    """Seeded walk: per frame a list of ((K,2) int32 key-points, confidence).  People leave and return, newcomers arrive,
    some confidences are equal (stable order), one pose has no key-point at all."""
    rng = np.random.RandomState(seed)
    cols = int(np.ceil(np.sqrt(n_people * 2)))
    cell = 90
    slots = rng.permutation(cols * cols)[:n_people + 3]
    origin = np.stack([(slots % cols) * cell + 60, (slots // cols) * cell + 60], 1)[:, None, :]
    shape = rng.randint(-30, 31, size=(n_people + 3, K, 2))
    vel = rng.randint(-5, 6, size=(n_people + 3, 1, 2))
    conf = np.round(rng.rand(n_people + 3) * 10, 3)
    if equal_conf:
        conf[1::4] = conf[0]                                           # a quarter of the crowd shares one confidence
    away = {t: set(rng.choice(n_people, size=max(1, n_people // 8), replace=False).tolist()) for t in range(2, n_frames, 3)}
    frames = []
    for t in range(n_frames):
        cur = []
        present = [p for p in rng.permutation(n_people) if p not in away.get(t, ())]
        if t >= 3:
            present.append(n_people)                                    # newcomers
        if t >= 5:
            present.append(n_people + 1)
        for p in present:
            kp = (origin[p] + shape[p] + vel[p] * t + rng.randint(-2, 3, size=(K, 2))).astype(np.int32)
            kp[rng.rand(K) < 0.15] = -1
            if strangers and t == 4 and p % 5 == 0:
                kp = np.where(kp != -1, kp + 9000, kp).astype(np.int32)  # similar to nobody
            cur.append((kp, float(conf[p])))
        if t in (1, 6):
            cur.insert(len(cur) // 2, (-np.ones((K, 2), np.int32), float(conf[0])))   # no key-point at all
        frames.append(cur)
    return frames


def run_tracking(ns, spy, frames, K, sigmas, match_threshold, smooth, sim_threshold):
    Pose, track, sim = ns["Pose"], ns["track_poses"], ns["get_similarity"]
    Pose.num_kpts = K
    Pose.sigmas = sigmas
    Pose.vars = (sigmas * 2) ** 2
    assert Pose.vars.dtype == np.float32
    sim.__defaults__ = (sim_threshold,)
    spy.threshold = sim_threshold
    Pose.last_id = -1
    prev, rec = [], []
    inherited = fresh_later = moved = 0
    for t, cur in enumerate(frames):
        poses = [Pose(kp.copy(), c) for kp, c in cur]
        before = Pose.last_id
        prev_ids = set(p.id for p in prev)
        with np.errstate(over="ignore"):
            track(prev, poses, threshold=match_threshold, smooth=smooth)
        inherited += sum(1 for p in poses if p.id in prev_ids)
        if t > 0:
            fresh_later += Pose.last_id - before
        moved += sum(int((p.keypoints != kp).sum()) for p, (kp, _) in zip(poses, cur))
        rec.append((poses, int(Pose.last_id)))
        prev = poses
    return rec, inherited, fresh_later, moved


def gen_tracking():
    ns = ref_pose_namespace()
    spy = NpSpy()
    ns["np"] = spy                                   # the parsed functions look `np` up in their globals
    coco = ns["Pose"].sigmas.copy()
    assert coco.dtype == np.float32 and coco.shape == (18,)
    sig5 = (np.array([.5, .9, .8, .8, .3], dtype=np.float32) / 10.0)
    sig21 = (np.array([.9] + [.6, .5, .4, .35] * 5, dtype=np.float32) / 10.0)
    # (file, case, seed, people, K, sigmas, match_threshold, smooth, similarity_threshold, strangers)
    plan = []
    for people, tag in ((35, "crowd35"), (70, "crowd70"), (150, "crowd150")):
        for smooth in (0, 1):
            plan.append((tag, "%s_%s" % (tag, "smooth" if smooth else "plain"), 100 + people, people, 18, coco, 3, smooth, 0.5, False))
    for thr in (1, 0, -1, 19):
        plan.append(("thresholds", "match%d" % thr, 300 + thr, 35, 18, coco, thr, 1, 0.5, True))
    for st in (0.1, 0.9):
        for smooth in (0, 1):
            plan.append(("thresholds", "sim%02d_%s" % (round(st * 10), "smooth" if smooth else "plain"), 320, 35, 18, coco, 3, smooth, st, False))
    for smooth in (0, 1):
        plan.append(("skeletons", "guide5_%s" % ("smooth" if smooth else "plain"), 405, 12, 5, sig5, 3, smooth, 0.5, False))
        plan.append(("skeletons", "hand21_%s" % ("smooth" if smooth else "plain"), 421, 12, 21, sig21, 3, smooth, 0.5, False))
    files = {}
    for fname, case, seed, people, K, sigmas, thr, smooth, st, strangers in plan:
        frames = crowd(seed, 8, people, K, strangers=strangers)
        rec, inherited, fresh_later, moved = run_tracking(ns, spy, frames, K, sigmas, thr, bool(smooth), st)
        # what the case is for.  match_threshold above K cannot be met (a pose has K key-points): nothing may be inherited then
        if thr > K:
            assert inherited == 0, (case, inherited)
        else:
            assert inherited > 0, case
        assert fresh_later > 0, case
        # smoothing moves a coordinate only through an inherited filter (a fresh filter returns its input)
        assert (moved > 0) == (bool(smooth) and thr <= K), (case, moved)
        assert max(len(f) for f in frames) >= people - people // 8, case
        d = files.setdefault(fname, {})
        d[case + ":meta"] = np.array([K, thr, smooth, len(frames)], np.int32)
        d[case + ":similarity_threshold"] = np.array(st, np.float64)
        d[case + ":sigmas"] = sigmas
        d[case + ":n"] = np.array([len(f) for f in frames], np.int32)
        d[case + ":in_kp"] = np.concatenate([np.stack([kp for kp, _ in f]) for f in frames]).astype(np.int32)
        d[case + ":in_conf"] = np.array([c for f in frames for _, c in f], np.float64)
        d[case + ":out_kp"] = np.concatenate([np.stack([p.keypoints for p in poses]) for poses, _ in rec]).astype(np.int32)
        d[case + ":out_bbox"] = np.array([p.bbox for poses, _ in rec for p in poses], np.int32).reshape(-1, 4)
        d[case + ":out_ids"] = np.array([p.id for poses, _ in rec for p in poses], np.int32)
        d[case + ":last_id"] = np.array([l for _, l in rec], np.int32)
    for fname, d in files.items():
        d["cases"] = np.array(sorted(k[:-5] for k in d if k.endswith(":meta")))
        save(fname, d)
    print("smallest |exp(-q) - similarity_threshold| met: %.3e" % spy.closest)
    assert spy.closest > 1e-9, spy.closest


# ------------------------------------------------------------------------------------------------ un-map + pose rows
# (name, (n_people, h, w, seed, drop_prob, noise), upsample_ratio, stride, scale, pad_top, pad_left); pads "kp<i>" are derived
# from key-point row i so that it un-maps to exactly -1
UNMAP_CASES = [
    ("identity", (5, 46, 82, 4, 0.15, 0.02), 4, 8, 1.0, 0, 0),
    ("demo_like", (5, 46, 82, 4, 0.15, 0.02), 4, 8, 0.5111111111111111, 0, 3),
    ("big_scale", (4, 46, 82, 9, 0.1, 0.02), 4, 8, 7.3, 2, 5),
    ("small_scale", (4, 46, 82, 9, 0.1, 0.02), 4, 8, 0.013, 1, 1),
    ("pad_negative", (5, 46, 82, 4, 0.15, 0.02), 4, 8, 0.37, 150, 290),
    ("minus_one_x", (5, 46, 82, 4, 0.15, 0.02), 4, 8, 1.0, 7, "kp3x"),
    ("minus_one_y", (5, 46, 82, 4, 0.15, 0.02), 4, 8, 1.0, "kp3y", 11),
    ("ratio8_stride3", (2, 16, 24, 7, 0.0, 0.01), 8, 3, 1.7, 5, 9),
    ("ratio8_stride7", (2, 16, 24, 7, 0.0, 0.01), 8, 7, 0.61, 13, 40),
]


def gen_unmap():
    ns = ref_pose_namespace()
    Pose = ns["Pose"]
    code = demo_tail_loops()
    d = {"cases": np.array([c[0] for c in UNMAP_CASES])}
    for name, mp, ratio, stride, scale, pad_top, pad_left in UNMAP_CASES:
        heat, paf, _ = synth.make_pose_maps(*mp)
        hu = post_ref.upsample_cubic(heat.transpose(1, 2, 0), ratio)
        pu = post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)
        by_type, total = [], 0
        for k in range(18):
            total += post_ref.extract_keypoints(hu[:, :, k], by_type, total)
        ent, allk = post_ref.group_keypoints(by_type, pu, demo=True)
        ent = np.asarray(ent, np.float64).reshape(-1, 20)
        allk = np.asarray(allk, np.float64).reshape(-1, 4)
        used = int(ent[0, :18][ent[0, :18] >= 0][3])                    # a key-point row that pose 0 uses
        if pad_left == "kp3x":
            pad_left = int(allk[used, 0] * stride / ratio) + 1
        if pad_top == "kp3y":
            pad_top = int(allk[used, 1] * stride / ratio) + 1
        env = {"np": np, "Pose": Pose, "all_keypoints": allk.copy(), "pose_entries": ent.copy(), "stride": stride,
               "upsample_ratio": ratio, "pad": [pad_top, pad_left, 0, 0], "scale": scale, "num_keypoints": 18}
        exec(code, env)
        poses = env["current_poses"]
        assert len(poses) == len(ent) >= 2, name
        kp = np.stack([p.keypoints for p in poses]).astype(np.int32)
        if name.startswith("minus_one"):
            col = 0 if name.endswith("x") else 1
            real = ent[:, :18] != -1.0
            assert np.any((kp[:, :, col] == -1) & real), name           # a real coordinate truncated to exactly -1
        if name == "pad_negative":
            assert (kp < -1).any(), name
        d[name + ":maps"] = np.array(mp, np.float64)
        d[name + ":geometry"] = np.array([ratio, stride, pad_top, pad_left], np.int32)
        d[name + ":scale"] = np.array(scale, np.float64)
        d[name + ":entries"] = ent
        d[name + ":all_keypoints"] = allk
        d[name + ":out_kp"] = kp
        d[name + ":out_conf"] = np.array([p.confidence for p in poses], np.float64)
        d[name + ":out_bbox"] = np.array([p.bbox for p in poses], np.int32).reshape(-1, 4)
    save("unmap", d)


if __name__ == "__main__":
    gen_unmap()
    gen_tracking()
