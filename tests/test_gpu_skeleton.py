"""Custom skeletons on the GPU (-m gpu): lwp_set_skeleton + the generic grouping kernels against the reference's own outputs
(tests/golden/skeleton_*.npz) and the oracle with patched tables.  Every comparison is bit-exact: (n,4) key-points,
(P,E) pose entries, per-type counts — the bar of the existing post-processing tests."""
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth, workload
from lwpose_amd._lib import CapacityError
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules import keypoints as kp_mod
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine
from oracle import post_ref

import skeleton_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MAP_NAMES = [c[0] for c in sc.MAP_CASES] + [c[0] for c in sc.OPTION_CASES]
POST = ["p1_small", "p3_small", "p0_empty", "p5_mid", "p10_full", "p4_noisy", "p2_r8"]


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def case_maps(name):
    if name.startswith("coco_options"):
        heat, paf = sc.option_maps([c[1] for c in sc.OPTION_CASES if c[0] == name][0])
    else:
        heat, paf = sc.make_maps(sc.map_case(name))
    return heat, paf


def skeleton_engine(g, NH, NP):
    e = Engine(0, num_heatmaps=NH, num_pafs=NP)
    e.set_skeleton(g["limb_kpts"].tolist(), g["limb_pafs"].tolist(), int(g["K"]), int(g["pose_entry_size"]), float(g["min_paf_score"]))
    return e


def counts_of(kp, K):
    return np.bincount(kp[:, 4].astype(int), minlength=K) if len(kp) else np.zeros(K, int)


def check(res, g, tag, K):
    ent, allk, counts = res
    E = int(g["pose_entry_size"])
    assert np.array_equal(allk, g[tag + "_allk"].reshape(-1, 4)), tag
    assert np.array_equal(counts, counts_of(g[tag + "_kp"], K)), tag
    assert ent.shape[1] == E
    assert np.array_equal(ent, g[tag + "_entries"].reshape(-1, E)), tag


def oracle_post(monkeypatch, hu, pu, K, kpts, pafs, demo, E=20, mp=0.05):
    """(entries (P,E), all_keypoints (n,4), counts (K,)) of the oracle with the tables patched, on up-sampled HWC maps."""
    monkeypatch.setattr(post_ref, "KPT_IDS", [list(p) for p in kpts])
    monkeypatch.setattr(post_ref, "PAF_IDS", [list(p) for p in pafs])
    heat = np.array(hu, dtype=np.float32)
    by_type, total = [], 0
    for k in range(K):
        total += post_ref.extract_keypoints(heat[:, :, k], by_type, total)
    ent, allk = post_ref.group_keypoints(by_type, pu, pose_entry_size=E, min_paf_score=mp, demo=demo)
    return np.asarray(ent, dtype=np.float64).reshape(-1, E), np.asarray(allk, dtype=np.float64).reshape(-1, 4), counts_of(sc.flat_kp(by_type), K)


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def same_all(a, b):
    return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------ 1. goldens through every entry point
@pytest.mark.parametrize("name", MAP_NAMES)
def test_skeleton_golden_through_every_entry_point(monkeypatch, name):
    g = load("skeleton_%s.npz" % name)
    K, ratio, E = int(g["K"]), int(g["ratio"]), int(g["pose_entry_size"])
    heat, paf = case_maps(name)
    eng = skeleton_engine(g, heat.shape[0], paf.shape[0])
    assert eng.post_generic                                   # a custom skeleton (or options) runs the generic kernels
    hu = post_ref.upsample_cubic(heat.transpose(1, 2, 0), ratio)
    pu = post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)
    kpts, pafs = g["limb_kpts"].tolist(), g["limb_pafs"].tolist()
    monkeypatch.setattr(kp_mod, "BODY_PARTS_KPT_IDS", kpts)
    monkeypatch.setattr(kp_mod, "BODY_PARTS_PAF_IDS", tuple(pafs))
    d_eng = Engine(0, num_heatmaps=heat.shape[0], num_pafs=paf.shape[0])     # the drop-in pushes the tables itself
    for tag, demo in (("demo", True), ("val", False)):
        check(eng.poses_from_maps(heat[None], paf[None], ratio, demo)[0], g, tag, K)
        check(eng.poses_from_maps(hu[None], pu[None], 1, demo, layout="NHWC")[0], g, tag, K)
        gk = g[tag + "_kp"]
        ent = eng.group_keypoints(gk[:, :4], counts_of(gk, K), pu, demo)
        assert np.array_equal(ent, g[tag + "_entries"].reshape(-1, E)), tag
        d_ent, d_allk = kp_mod.group_keypoints(sc.by_type_from_flat(gk, K), pu, pose_entry_size=E,
                                               min_paf_score=float(g["min_paf_score"]), demo=demo, engine=d_eng)
        assert tuple(np.asarray(d_ent).shape) == tuple(g[tag + "_entries_shape"]), tag
        assert np.array_equal(d_ent, g[tag + "_entries"]) and np.array_equal(d_allk, g[tag + "_allk"]), tag


# ------------------------------------------------------------------------------------------ 1 + 5. hand-made lists, large forms
def test_skeleton_adversarial_golden_and_large_forms(monkeypatch):
    """Hand-made lists through lwp_group_keypoints and the drop-in.  lwp_debug_post_counts_ex shows that the '> 64' cases ran
    the non-register forms of the generic match (81 candidates on one limb; > 64 on both limbs of 'spill', where samples
    of crossing pairs land on other people's field columns) and the spilled rows of the generic
    assembly (70 surviving entries: entries 64.. live past its 64 LDS rows)."""
    g = load("skeleton_adversarial.npz")
    for name, (K, kpts, pafs, bt, paf) in sc.adversarial_cases().items():
        E = max(20, K + 2)
        eng = Engine(0, num_heatmaps=K + 1, num_pafs=paf.shape[2])
        eng.set_skeleton(kpts, pafs, K, E)
        d_eng = Engine(0, num_heatmaps=K + 1, num_pafs=paf.shape[2])
        monkeypatch.setattr(kp_mod, "BODY_PARTS_KPT_IDS", kpts)
        monkeypatch.setattr(kp_mod, "BODY_PARTS_PAF_IDS", pafs)
        kp = sc.flat_kp(bt)
        for tag, demo in (("demo", True), ("val", False)):
            key = "%s:%s" % (name, tag)
            ent = eng.group_keypoints(kp[:, :4], counts_of(kp, K), paf, demo)
            assert np.array_equal(ent, g["ent:" + key].reshape(-1, E)), key
            cand, picked = eng.post_counts(0)[2:]
            if name == "many_candidates":
                assert cand[0] == 81 and picked[0] == 9, (cand, picked)
            if name == "spill":
                assert min(cand) > 64 and picked.tolist() == [70, 70] and len(ent) == 70, (cand, picked, len(ent))
            d_ent, _ = kp_mod.group_keypoints([list(l) for l in bt], paf, pose_entry_size=E, demo=demo, engine=d_eng)
            assert tuple(np.asarray(d_ent).shape) == tuple(g["ent_shape:" + key]), key
            assert np.array_equal(np.asarray(d_ent, dtype=np.float64), g["ent:" + key]), key


# ------------------------------------------------------------------------------------------ 2. LWP_POST_GENERIC=1, default skeleton
@pytest.fixture(scope="module")
def generic_eng():
    old = os.environ.get("LWP_POST_GENERIC")
    os.environ["LWP_POST_GENERIC"] = "1"
    try:
        return Engine(0)
    finally:
        if old is None:
            del os.environ["LWP_POST_GENERIC"]
        else:
            os.environ["LWP_POST_GENERIC"] = old


def test_generic_switch_selects_the_generic_kernels(generic_eng):
    """LWP_POST_GENERIC=1 is what makes the tests below compare the generic kernels (and not the specialised ones twice)."""
    assert generic_eng.post_generic
    assert not Engine(0).post_generic
    heat, paf, _ = synth.make_pose_maps(2, 16, 24, 7, 0.0, 0.01)
    generic_eng.poses_from_maps(heat[None], paf[None], 8, True)
    assert generic_eng.post_generic                           # the workspace it ran with


@pytest.mark.parametrize("name", POST)
def test_generic_forms_reproduce_coco_post_goldens(generic_eng, name):
    g = np.load(os.path.join(GOLDEN, "post_%s.npz" % name))
    n, h, w, seed, ratio = [int(v) for v in g["params"]]
    heat, paf, _ = synth.make_pose_maps(n, h, w, seed, float(g["drop"]), float(g["noise"]))
    pu = post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)
    for tag, demo in (("demo", True), ("val", False)):
        ent, allk, counts = generic_eng.poses_from_maps(heat[None], paf[None], ratio, demo)[0]
        gk = g[tag + "_kp"]
        assert np.array_equal(allk, g[tag + "_allk"].reshape(-1, 4))
        assert np.array_equal(counts, counts_of(gk, 18))
        assert np.array_equal(ent.reshape(-1, 20), g[tag + "_entries"].reshape(-1, 20))
        ent2 = generic_eng.group_keypoints(gk[:, :4], counts_of(gk, 18), pu, demo)
        assert np.array_equal(ent2.reshape(-1, 20), g[tag + "_entries"].reshape(-1, 20))


def test_generic_forms_reproduce_group_adversarial_golden(generic_eng):
    g = np.load(os.path.join(GOLDEN, "group_adversarial.npz"))
    for nm in [k[4:] for k in g.files if k.startswith("paf:")]:
        kp = g["kp:" + nm]
        for tag, demo in (("demo", True), ("val", False)):
            ent, _ = kp_mod.group_keypoints(sc.by_type_from_flat(kp, 18), g["paf:" + nm], demo=demo, engine=generic_eng)
            key = "%s:%s" % (nm, tag)
            assert tuple(np.asarray(ent).shape) == tuple(g["ent_shape:" + key]), key
            assert np.array_equal(np.asarray(ent, dtype=np.float64), g["ent:" + key]), key


def test_generic_forms_equal_specialised_on_calibrated_bench_frames(generic_eng):
    net, _ = workload.build_net(nref=1, seed=1, device=0)
    x = workload.normalized_input(synth.make_frames(4, 368, 656, seed0=0))
    outs = net.engine.forward(x)
    for demo in (True, False):
        spec = net.engine.poses_from_maps(outs[-2], outs[-1], 4, demo)
        gen = generic_eng.poses_from_maps(outs[-2], outs[-1], 4, demo)
        assert sum(len(r[0]) for r in spec) >= 4
        assert same_all(spec, gen)


# ------------------------------------------------------------------------------------------ 3. end to end on the network
def custom_net(NH, NP, kpts, pafs, seed):
    sd = synth.make_state_dict(1, seed=seed, num_heatmaps=NH, num_pafs=NP)
    net = PoseEstimationWithMobileNet(num_refinement_stages=1, num_heatmaps=NH, num_pafs=NP)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    outs = net(workload.normalized_input(synth.make_frames(1, 184, 328, seed0=0)))
    sd = synth.calibrate_heads(sd, outs[-2][0], outs[-1][0], 1)
    load_state(net, {"state_dict": sd})
    net.cuda()
    net.engine.set_skeleton(kpts, pafs, NH - 1)
    return net


@pytest.mark.parametrize("NH,NP,kpts,pafs", [(6, 8, sc.GUIDE5_KPTS, sc.GUIDE5_PAFS), (22, 40, sc.HAND21_KPTS, sc.HAND21_PAFS)],
                         ids=["guide5", "hand21"])
def test_end_to_end_custom_network(monkeypatch, NH, NP, kpts, pafs):
    K = NH - 1
    E = max(20, K + 2)
    net = custom_net(NH, NP, kpts, pafs, seed=21)
    eng = net.engine
    frames = synth.make_frames(3, 184, 328, seed0=30)
    x = workload.normalized_input(frames)
    res = eng.infer_poses(x, 4, demo=True)
    outs = eng.forward(x)
    assert same_all(res, eng.poses_from_maps(outs[-2], outs[-1], 4, True))
    for f in range(3):
        hu = post_ref.upsample_cubic(outs[-2][f].transpose(1, 2, 0), 4)
        pu = post_ref.upsample_cubic(outs[-1][f].transpose(1, 2, 0), 4)
        assert same(res[f], oracle_post(monkeypatch, hu, pu, K, kpts, pafs, True, E)), f
    assert sum(int(r[2].sum()) for r in res) > 0 and sum(len(r[0]) for r in res) >= 1
    assert eng.post_generic
    xd = torch.from_numpy(x).cuda()
    eng.infer_poses_async(xd, 4, demo=True)
    assert same_all(res, eng.fetch_poses())
    eng.pipeline_submit(xd, 0, 4, demo=True)
    assert same_all(res, eng.pipeline_fetch(0))
    # multi-scale (val.infer_batch + poses_batch) == the patched oracle on the same averaged maps
    from lwpose_amd.val import infer_batch, poses_batch
    ah, ap = infer_batch(net, frames, [0.5, 1.0, 1.5], 184, 8)
    got = poses_batch(net, ah, ap)
    ah, ap = ah.cpu().numpy(), ap.cpu().numpy()
    for f in range(3):
        assert same(got[f], oracle_post(monkeypatch, ah[f], ap[f], K, kpts, pafs, False, E)), f


# ------------------------------------------------------------------------------------------ 4. switching skeletons on one handle
def test_switching_skeletons_and_batch_equals_single_frames():
    eng = Engine(0, num_heatmaps=22, num_pafs=40)
    heat, paf, _ = synth.make_pose_maps(5, 46, 82, 4, 0.15, 0.02)
    hc = np.zeros((1, 22, 46, 82), np.float32); hc[0, :19] = heat
    pc = np.zeros((1, 40, 46, 82), np.float32); pc[0, :38] = paf
    first = eng.poses_from_maps(hc, pc, 4, True)
    assert len(first[0][0]) >= 2
    g5 = load("skeleton_guide5_r4.npz")
    h5, p5 = case_maps("guide5_r4")
    eng.set_skeleton(sc.GUIDE5_KPTS, sc.GUIDE5_PAFS, 5)
    h5c = np.zeros((1, 22) + h5.shape[1:], np.float32); h5c[0, :6] = h5
    p5c = np.zeros((1, 40) + p5.shape[1:], np.float32); p5c[0, :8] = p5
    check(eng.poses_from_maps(h5c, p5c, 4, True)[0], g5, "demo", 5)
    gh = load("skeleton_hand21.npz")
    hh, ph = case_maps("hand21")
    eng.set_skeleton(sc.HAND21_KPTS, sc.HAND21_PAFS, 21)
    check(eng.poses_from_maps(hh[None], ph[None], 4, True)[0], gh, "demo", 21)
    # 32 frames in one call == 32 single-frame calls (the frames differ: the hand maps rolled along x)
    hb = np.stack([np.roll(hh, 3 * i, axis=2) for i in range(32)])
    pb = np.stack([np.roll(ph, 3 * i, axis=2) for i in range(32)])
    batch = eng.poses_from_maps(hb, pb, 4, False)
    singles = [eng.poses_from_maps(hb[i:i + 1], pb[i:i + 1], 4, False)[0] for i in range(32)]
    assert sum(len(r[0]) for r in batch) >= 32
    assert same_all(batch, singles)
    eng.set_skeleton(None, None)
    assert eng.skeleton["num_kpt_types"] == 18 and eng.skeleton["pose_entry_size"] == 20
    assert same_all(first, eng.poses_from_maps(hc, pc, 4, True))
    assert not eng.post_generic


def test_changing_the_skeleton_discards_an_unfetched_async_run():
    """lwp_set_skeleton / lwp_set_capacity re-size the workspace an lwp_infer_poses_async run left its results in: a later
    lwp_fetch_poses must report LWP_ERR_STATE (RuntimeError), not read the freed workspace."""
    net = custom_net(6, 8, sc.GUIDE5_KPTS, sc.GUIDE5_PAFS, seed=21)
    eng = net.engine
    xd = torch.from_numpy(workload.normalized_input(synth.make_frames(2, 184, 328, seed0=30))).cuda()
    ref = eng.infer_poses(xd, 4, demo=True)
    eng.infer_poses_async(xd, 4, demo=True)
    assert same_all(ref, eng.fetch_poses())
    for change in (lambda: eng.set_skeleton(sc.GUIDE5_KPTS[:3], sc.GUIDE5_PAFS[:3], 5), lambda: eng.set_capacity()):
        eng.infer_poses_async(xd, 4, demo=True)
        change()
        with pytest.raises(RuntimeError, match="no pipeline run to fetch"):
            eng.fetch_poses()
    eng.infer_poses_async(xd, 4, demo=True)                   # a new run fetches normally (3-limb skeleton now)
    assert len(eng.fetch_poses()) == 2


# ------------------------------------------------------------------------------------------ 6. errors through the Python layer
def test_errors_capacity_unbound_validation_and_run_demo():
    K, kpts, pafs, bt, paf = sc.adversarial_cases()["spill"]
    eng = Engine(0, num_heatmaps=4, num_pafs=4)
    eng.set_skeleton(kpts, pafs, K)
    eng.set_capacity(max_entries=32)
    kp = sc.flat_kp(bt)
    with pytest.raises(CapacityError):
        eng.group_keypoints(kp[:, :4], counts_of(kp, K), paf, True)
    eng.set_capacity()
    nanpaf = paf.copy()
    nanpaf[:, :, 1] = np.nan                                   # every mid-point of limb 0 fails '> -100' before any passes
    with pytest.raises(UnboundLocalError):
        eng.group_keypoints(kp[:, :4], counts_of(kp, K), nanpaf, True)
    for args in [dict(num_kpt_types=0), dict(num_kpt_types=65), dict(num_kpt_types=5), dict(pose_entry_size=4),
                 dict(pose_entry_size=257)]:
        with pytest.raises(ValueError):
            eng.set_skeleton(kpts, pafs, **args)
    for kt, pt in [([], []), ([[0, 1]] * 321, [[0, 1]] * 321), ([[0, 3]], [[0, 1]]), ([[1, 1]], [[0, 1]]), ([[0, 1]], [[0, 4]]),
                   ([[-1, 1]], [[0, 1]]), ([[0, 1]], [[-1, 1]])]:
        with pytest.raises(ValueError):
            eng.set_skeleton(kt, pt, 3)
    assert eng.skeleton["num_kpt_types"] == 3 and eng.skeleton["limb_kpts"].tolist() == kpts   # refused calls change nothing
    from lwpose_amd.demo import run_demo

    class _Net(object):
        engine = eng
    with pytest.raises(ValueError, match="key-point types"):
        run_demo(_Net(), [], 368, False, False, False)
