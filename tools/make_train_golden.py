"""Generates tests/golden/train_targets.npz, train_targets_custom.npz, train_targets_grid.npz, train_loss.npz and
train_loss_grid.npz: the reference's own target rendering (datasets/coco.py _generate_keypoint_maps / _add_gaussian / _generate_paf_maps / _set_paf) and its l2_loss
(modules/loss.py) on the cases of tests/train_cases.py.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_train_golden.py

The reference's statements are executed, not restated.  datasets/coco.py cannot be imported (it imports cv2 and
pycocotools), so the four methods are taken out of its syntax tree and compiled as plain functions whose ``self`` is a small
object with ``_stride`` / ``_sigma`` / ``_paf_thickness``.  A custom key-point set is bound the way TRAIN-ON-CUSTOM-DATASET.md
tells a user to edit the file: the module's ``BODY_PARTS_KPT_IDS`` is the new limb list (row j owns PAF channels 2j, 2j + 1),
and the literal 18 assigned to ``n_keypoints`` becomes the new count (the synthetic chains of train_targets_grid.npz too).  ``l2_loss`` runs in torch float32 on the CPU.  The
files hold data only: every case's inputs and the arrays the reference made of them."""
import ast
import io
import math
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("LWP_REFERENCE", "/root/reference")

import lwpose_amd  # noqa: E402,F401
import train_cases as tc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
METHODS = ("_generate_keypoint_maps", "_add_gaussian", "_generate_paf_maps", "_set_paf")


def save(name, d):
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:       # fixed dates: two runs give identical files
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 900 * 1024, (path, os.path.getsize(path))
    print("%8d  %s" % (os.path.getsize(path), os.path.basename(path)))


def ref_target_namespace(K, limbs):
    """The four methods of the reference's CocoTrainDataset as functions of a namespace with the given tables."""
    tree = ast.parse(open(os.path.join(REF, "datasets", "coco.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "CocoTrainDataset"][0]
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in METHODS]
    assert sorted(f.name for f in fns) == sorted(METHODS)
    edits = 0
    for f in fns:
        for n in ast.walk(f):
            if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "n_keypoints":
                assert isinstance(n.value, ast.Constant) and n.value.value == 18
                n.value = ast.Constant(K)
                edits += 1
    assert edits == 1
    mod = ast.Module(fns, [])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "math": math, "BODY_PARTS_KPT_IDS": [list(l) for l in limbs]}
    exec(compile(mod, os.path.join(REF, "datasets", "coco.py"), "exec"), ns)
    return ns


class Self(object):
    def __init__(self, ns, stride, sigma, thickness):
        self._stride, self._sigma, self._paf_thickness = stride, sigma, thickness
        for m in METHODS:
            setattr(self, m, ns[m].__get__(self))


def ref_l2_loss():
    tree = ast.parse(open(os.path.join(REF, "modules", "loss.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "l2_loss"]
    mod = ast.Module(fn, [])
    ast.fix_missing_locations(mod)
    ns = {}
    exec(compile(mod, os.path.join(REF, "modules", "loss.py"), "exec"), ns)
    return ns["l2_loss"]


def gen_targets():
    cases = tc.all_cases()
    files = tc.TARGET_FILES
    got = {}
    for fname, names in files.items():
        d = {"cases": np.array(names)}
        for name in names:
            skel, H, W, stride, sigma, thick, frames = cases[name]
            K, limb_kpts, limb_pafs = tc.skeleton(skel)
            if skel == "coco":
                ref_limbs = tc.train_limbs(limb_kpts, limb_pafs)
                ref_ns = ref_target_namespace(18, ref_limbs)
                src = open(os.path.join(REF, "datasets", "coco.py")).read()
                assert ref_limbs == ast.literal_eval(src[src.index("BODY_PARTS_KPT_IDS = ") + 21:src.index("\n\n\ndef get_mask")])
            elif skel.startswith("chain"):              # synthetic chains: limb j = (j, j + 1), bound the same way
                ref_limbs = tc.train_limbs(limb_kpts, limb_pafs)
                assert ref_limbs == [[j, j + 1] for j in range(K - 1)]
                ref_ns = ref_target_namespace(K, ref_limbs)
            else:                                       # the tables of the custom-skeleton fixtures, bound as the guide says
                g = np.load(os.path.join(OUT, "skeleton_hand21.npz" if skel == "hand21" else "skeleton_guide5_r4.npz"))
                assert g["limb_kpts"].tolist() == [list(p) for p in limb_kpts] and g["limb_pafs"].tolist() == [list(p) for p in limb_pafs]
                assert int(g["K"]) == K
                ref_ns = ref_target_namespace(K, tc.train_limbs(g["limb_kpts"].tolist(), g["limb_pafs"].tolist()))
            me = Self(ref_ns, stride, sigma, thick)
            kmaps, pmaps = [], []
            for label in tc.frames_to_labels(frames, K):
                sample = {"image": np.zeros((H, W, 3), np.uint8), "label": label}
                kmaps.append(me._generate_keypoint_maps(sample))
                pmaps.append(me._generate_paf_maps(sample))
            kmaps, pmaps = np.stack(kmaps), np.stack(pmaps)
            assert kmaps.dtype == np.float32 and pmaps.dtype == np.float32
            assert kmaps.shape == (len(frames), K + 1, H // stride, W // stride) and pmaps.shape[1] == 2 * len(limb_kpts)
            kpts, n = tc.frames_to_arrays(frames, K)
            d[name + ":geometry"] = np.array([H, W, stride, K], np.int32)
            d[name + ":sigma_thickness"] = np.array([sigma, thick], np.float64)
            d[name + ":kpts"] = kpts
            d[name + ":n_persons"] = n
            d[name + ":keypoint_maps"] = kmaps
            d[name + ":paf_maps"] = pmaps
            got[name] = (kmaps, pmaps, frames)
        save(fname, d)
    # what each case is for
    k, p, fr = got["borders"]
    assert k[0, 0, 0, 0] == 1.0                                        # the key-point on a cell centre
    assert (k[0, :18] == 1.0).sum() > 3                                # the clip fired
    assert not k[1, :18].any() and (k[1, 18] == 1).all() and not p[1].any()     # nobody: zero maps, background 1
    me = Self(ref_target_namespace(18, tc.COCO_TRAIN_LIMBS), 8, 7, 1)   # person b of frame 0 alone: one special key-point per channel
    kb = me._generate_keypoint_maps({"image": np.zeros((48, 40, 3), np.uint8), "label": tc.frames_to_labels([[fr[0][1]]], 18)[0]})
    assert kb[1].any() and kb[2].any() and kb[3].any() and not kb[4].any() and not kb[5].any() and kb[6].any() and kb[7].any()
    k, p, _ = got["paf_t1"]
    assert p[0, 12, 1, 2] == 1.0 and p[0, 12, 2, 2] == 1.0 and p[0, 12, 3, 2] == 0.0 and p[0, 12, 0, 2] == 0.0   # row 1: d == thickness counts; row 3: outside the box
    assert not p[0, 0:2].any() and not p[0, 20:22].any()               # zero length; an end with visibility 2
    assert p[0, 6:8].any() and p[0, 22:24].any() and p[0, 34:36].any()  # partly outside; the second person's limbs
    assert (got["paf_t2"][1] != 0).sum() > (p != 0).sum()
    a, b = got["cross_ab"][1], got["cross_ba"][1]
    assert not np.array_equal(a, b) and np.array_equal(a != 0, b != 0)  # the last person wins the crossing
    for name in ("chunk", "two_chunks_plus", "hand21"):
        assert max(len(f) for f in got[name][2]) > tc.CHUNK
    assert sorted(len(f) for f in got["chunk"][2]) == [tc.CHUNK - 1, tc.CHUNK, tc.CHUNK + 1]
    tc.check_grid_cases(cases, {name: got[name][:2] for name in tc.GRID_CASES})


def gen_loss(fname, stages):
    """``stages``: case name -> number of stages (two tensors each)."""
    l2 = ref_l2_loss()
    d = {"cases": np.array(sorted(stages))}
    for name in sorted(stages):
        n_stages = stages[name]
        outs, kt, pt, mask = tc.loss_inputs(name, n_stages)
        N = kt.shape[0]
        losses = []
        for i, o in enumerate(outs):
            t = pt if i % 2 else kt
            m = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(mask[:, None], t.shape)))
            v = l2(torch.from_numpy(o), torch.from_numpy(t), m, N)
            assert v.dtype == torch.float32
            losses.append(v.item())
        d[name + ":n_stages"] = np.array(n_stages, np.int32)
        d[name + ":losses_f32"] = np.array(losses, np.float32)
        d[name + ":digest"] = np.array([float(np.float64(o.astype(np.float64).sum())) for o in outs + [kt, pt, mask]])
    save(fname, d)


if __name__ == "__main__":
    gen_targets()
    gen_loss("train_loss", {name: 4 if name == "small" else 2 for name in tc.LOSS_CASES})
    gen_loss("train_loss_grid", {"s18": tc.LOSS_GRID_STAGES["s18"]})
