"""Record the augmentation fixtures tests/golden/augment_cases.npz from the REFERENCE's own Python.

    LWP_REFERENCE=/path/to/lightweight-human-pose-estimation.pytorch python tools/make_augment_golden.py

The reference's datasets/transformations.py is read at run time and executed unchanged (nothing of it is copied); the cv2 it
imports is a stand-in module built from this project's three pixel routines plus the flip, since cv2 itself is not
available.  So the fixtures pin everything the reference computes in Python — labels, sizes, crop geometry, the order of the
random draws, dtype conversions — while the pixel arithmetic is the project's own restatement of OpenCV (unpinned vs cv2).
Each case stores its inputs, its seed, the outputs and Python's ``random`` state after the reference ran.  No GPU needed.
"""
import copy
import json
import os
import random
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lwpose_amd  # noqa: E402,F401
from lwpose_amd.datasets import transformations as T  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "augment_cases.npz")
STRIDE, PAD, PERTURB, CASES = 8, (128, 128, 128), 6, 14


def standin_cv2():
    cv2 = types.ModuleType("cv2")
    cv2.BORDER_CONSTANT, cv2.INTER_LINEAR, cv2.INTER_AREA = 0, 1, 3

    def resize(src, dsize=None, fx=0, fy=0, interpolation=cv2.INTER_LINEAR):
        assert not dsize or tuple(dsize) == (0, 0)
        assert fx == fy
        if interpolation == cv2.INTER_AREA:
            return T.mask_small_u8(src, int(round(1 / fx)))
        return T.resize_linear(src, fx)

    def warpAffine(src, M, dsize, borderMode=None, borderValue=0):
        assert borderMode == cv2.BORDER_CONSTANT
        border = borderValue if src.ndim == 3 else np.asarray(borderValue).reshape(-1)[0]
        return T.warp_affine(src, M, dsize, border)

    cv2.resize, cv2.warpAffine = resize, warpAffine
    cv2.getRotationMatrix2D = T.rotation_matrix
    cv2.flip = lambda src, code: {1: T.flip_horizontal}[code](src)
    return cv2


def reference_module():
    path = os.path.join(os.environ["LWP_REFERENCE"], "datasets", "transformations.py")
    sys.modules["cv2"] = standin_cv2()
    mod = types.ModuleType("reference_transformations")
    with open(path) as f:
        exec(compile(f.read(), path, "exec"), mod.__dict__)
    return mod


def person(g, h, w, force_origin, force_outside):
    kps = [[float(g.uniform(-3, w + 3)), float(g.uniform(-3, h + 3)), int(g.integers(0, 3))] for _ in range(17)]
    if force_origin:
        kps[int(g.integers(0, 17))][:2] = [0, 0]
    if force_outside:
        kps[int(g.integers(0, 17))][:2] = [float(w + 2.5), float(-1.25)]
    return {"keypoints": kps, "objpos": [float(g.uniform(0.3, 0.7) * w), float(g.uniform(0.3, 0.7) * h)],
            "scale_provided": float(g.uniform(0.45, 0.9))}


def make_input(i):
    g = np.random.default_rng(7000 + i)
    h, w = int(g.integers(19, 41)), int(g.integers(19, 41))
    image = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    mask = np.ones((h, w), dtype=np.float32)
    y0, x0 = int(g.integers(0, h - 6)), int(g.integers(0, w - 6))
    mask[y0:y0 + int(g.integers(3, 12)), x0:x0 + int(g.integers(3, 12))] = 0
    mask[int(g.integers(0, h)), int(g.integers(0, w))] = 0.5
    label = person(g, h, w, i % 2 == 0, i % 3 == 0)
    label.update(img_width=w, img_height=h, img_paths="case%02d.jpg" % i,
                 processed_other_annotations=[person(g, h, w, False, True) for _ in range(i % 3)])
    return image, (None if i % 4 == 3 else mask), label


def main():
    ref = reference_module()
    out, i, kept = {}, 0, 0
    while kept < CASES:
        image, mask, label = make_input(i)
        crop_x, crop_y = (24, 16) if i % 2 == 0 else (16, 24)
        seed = 1000 + i
        i += 1
        transforms = [ref.ConvertKeypoints(), ref.Scale(), ref.Rotate(pad=PAD),
                      ref.CropPad(pad=PAD, center_perterb_max=PERTURB, crop_x=crop_x, crop_y=crop_y), ref.Flip()]
        sample = {"label": copy.deepcopy(label), "image": image.copy(),
                  "mask": np.ones(image.shape[:2], np.float32) if mask is None else mask.copy()}
        random.seed(seed)
        try:
            for t in transforms:
                sample = t(sample)
        except ValueError as e:                        # a crop the reference cannot assign: not a fixture
            print("seed %d: the reference raised %s" % (seed, e))
            continue
        state = random.getstate()
        assert sample["mask"].dtype == np.uint8 and sample["image"].dtype == np.uint8
        small = sys.modules["cv2"].resize(sample["mask"], dsize=None, fx=1 / STRIDE, fy=1 / STRIDE, interpolation=3)
        lab = sample["label"]
        people = [lab] + lab["processed_other_annotations"]
        k = "c%02d_" % kept
        out[k + "in_image"] = image
        out[k + "in_mask"] = np.zeros((0, 0), np.float32) if mask is None else mask
        out[k + "in_label"] = np.array(json.dumps(label))
        out[k + "seed"] = np.array(seed)
        out[k + "crop_xy"] = np.array([crop_x, crop_y])
        out[k + "image"] = sample["image"]
        out[k + "mask"] = sample["mask"]
        out[k + "mask_small"] = np.asarray(small, dtype=np.float32)
        out[k + "kpts"] = np.array([p["keypoints"] for p in people], dtype=np.float64)
        out[k + "objpos"] = np.array([p["objpos"] for p in people], dtype=np.float64)
        out[k + "img_wh"] = np.array([lab["img_width"], lab["img_height"]])
        out[k + "state"] = np.array(state[1], dtype=np.uint64)
        pad_share = float(np.all(sample["image"] == np.array(PAD, np.uint8), axis=2).mean())
        print("case %02d seed %d: %dx%d source, %d others, crop %dx%d, pad share %.2f, mask zeros %d" % (
            kept, seed, image.shape[0], image.shape[1], len(people) - 1, crop_y, crop_x, pad_share, int((sample["mask"] == 0).sum())))
        kept += 1
    out["n_cases"] = np.array(kept)
    out["stride"] = np.array(STRIDE)
    out["pad"] = np.array(PAD)
    out["center_perterb_max"] = np.array(PERTURB)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
