"""Generates tests/golden/skeleton_*.npz: the reference's own grouping (modules/keypoints.py extract_keypoints +
group_keypoints, with its two module tables set to a custom skeleton) on maps and key-point lists that repo code makes
from the parameters in tests/skeleton_cases.py.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_skeleton_golden.py

Only parameters, input digests and the reference's outputs are written; the tests regenerate the inputs.  The
reference's output must show what each case is for (asserted below), and two runs give identical files.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("LWP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth  # noqa: E402
from oracle import post_ref  # noqa: E402
import skeleton_cases as sc  # noqa: E402

from modules import keypoints as ref_kp  # noqa: E402  (reference)

OUT = os.path.join(ROOT, "tests", "golden")


def save(name, d):
    # np.savez_compressed stamps zip entries with the current time: write through a fixed-date ZipFile for identical files
    import io
    import zipfile
    path = os.path.join(OUT, "skeleton_%s.npz" % name)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 256 * 1024, path


def set_tables(kpts, pafs):
    ref_kp.BODY_PARTS_KPT_IDS = [list(p) for p in kpts]
    ref_kp.BODY_PARTS_PAF_IDS = tuple(list(p) for p in pafs)


def run_ref_maps(hu, pu, K, kpts, pafs, demo, pose_entry_size, min_paf_score):
    """demo.py:95-100 / val.py:129-134 with the module tables set, as TRAIN-ON-CUSTOM-DATASET.md asks."""
    set_tables(kpts, pafs)
    heat = hu.copy()
    by_type, total = [], 0
    for k in range(K):
        total += ref_kp.extract_keypoints(heat[:, :, k], by_type, total)
    ent, allk = ref_kp.group_keypoints(by_type, pu, pose_entry_size=pose_entry_size, min_paf_score=min_paf_score, demo=demo)
    return sc.flat_kp(by_type), np.asarray(ent, dtype=np.float64), np.asarray(allk, dtype=np.float64)


def gen_maps():
    for case in sc.MAP_CASES:
        name, canon, kpts, pafs, npafs, n, h, w, seed, drop, noise, ratio = case
        K = len(canon)
        E = max(20, K + 2)
        heat, paf = sc.make_maps(case)
        hu = post_ref.upsample_cubic(heat.transpose(1, 2, 0), ratio)
        pu = post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)
        d = {"lowres_digest": np.array(sc.digest(heat) + sc.digest(paf)), "up_digest": np.array(sc.digest(hu) + sc.digest(pu)),
             "K": np.array(K), "pose_entry_size": np.array(E), "min_paf_score": np.array(0.05), "ratio": np.array(ratio),
             "limb_kpts": np.array(kpts), "limb_pafs": np.array(pafs)}
        for demo in (True, False):
            kp, ent, allk = run_ref_maps(hu, pu, K, kpts, pafs, demo, E, 0.05)
            tag = "demo" if demo else "val"
            assert ent.ndim == 2 and len(ent) >= 2, (name, tag, ent.shape)
            if name == "hand21":       # limbs 17 / 18 (types 17 -> 18 -> 19) connected in some kept pose
                assert np.any((ent[:, 18] >= 0) & (ent[:, 19] >= 0)), (name, tag)
            d[tag + "_kp"], d[tag + "_entries"], d[tag + "_allk"] = kp, ent, allk
            d[tag + "_entries_shape"] = np.array(ent.shape)
        save(name, d)


def gen_options():
    for name, params, E, mp in sc.OPTION_CASES:
        ratio = params[-1]
        heat, paf = sc.option_maps(params)
        hu = post_ref.upsample_cubic(heat.transpose(1, 2, 0), ratio)
        pu = post_ref.upsample_cubic(paf.transpose(1, 2, 0), ratio)
        d = {"lowres_digest": np.array(sc.digest(heat) + sc.digest(paf)), "up_digest": np.array(sc.digest(hu) + sc.digest(pu)),
             "K": np.array(18), "pose_entry_size": np.array(E), "min_paf_score": np.array(mp), "ratio": np.array(ratio),
             "limb_kpts": np.array(sc.COCO_KPTS), "limb_pafs": np.array(sc.COCO_PAFS)}
        for demo in (True, False):
            kp, ent, allk = run_ref_maps(hu, pu, 18, sc.COCO_KPTS, sc.COCO_PAFS, demo, E, mp)
            tag = "demo" if demo else "val"
            assert ent.ndim == 2 and len(ent) >= 2 and ent.shape[1] == E, (name, tag, ent.shape)
            # the option must matter on these maps: the default threshold groups differently (ids, scores or counts)
            _, ent05, _ = run_ref_maps(hu, pu, 18, sc.COCO_KPTS, sc.COCO_PAFS, demo, E, 0.05)
            assert ent05.shape != ent.shape or not np.array_equal(ent05, ent), (name, tag)
            d[tag + "_kp"], d[tag + "_entries"], d[tag + "_allk"] = kp, ent, allk
            d[tag + "_entries_shape"] = np.array(ent.shape)
        save(name, d)


def gen_adversarial():
    d = {}
    for name, (K, kpts, pafs, bt, paf) in sc.adversarial_cases().items():
        set_tables(kpts, pafs)
        E = max(20, K + 2)
        d["paf_digest:" + name] = np.array(sc.digest(paf))
        d["kp:" + name] = sc.flat_kp(bt)
        for demo in (True, False):
            ent, allk = ref_kp.group_keypoints([list(l) for l in bt], paf, pose_entry_size=E, demo=demo)
            tag = "%s:%s" % (name, "demo" if demo else "val")
            d["ent:" + tag] = np.asarray(ent, dtype=np.float64)
            d["ent_shape:" + tag] = np.array(np.asarray(ent).shape)
            d["allk:" + tag] = np.asarray(allk, dtype=np.float64)
            if name == "spill":
                assert len(ent) > 64, len(ent)
    save("adversarial", d)


if __name__ == "__main__":
    gen_maps()
    gen_options()
    gen_adversarial()
    for f in sorted(os.listdir(OUT)):
        if f.startswith("skeleton_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
