"""Shared by test_augment_host.py and test_gpu_augment.py: the recorded reference runs of tests/golden/augment_cases.npz
(tools/make_augment_golden.py) and small synthetic samples.  Nothing here needs a GPU or the reference."""
import json
import os

import numpy as np

import lwpose_amd  # noqa: F401
from lwpose_amd.datasets import transformations as T

from conftest import GOLDEN

_FILE = None


def fixture_file():
    global _FILE
    if _FILE is None:
        _FILE = np.load(os.path.join(GOLDEN, "augment_cases.npz"))
    return _FILE


def n_cases():
    return int(fixture_file()["n_cases"])


def case(i):
    """(sample, transforms, seed, expected dict) of fixture case i; the sample is fresh at every call."""
    z, k = fixture_file(), "c%02d_" % i
    mask = z[k + "in_mask"]
    sample = {"image": z[k + "in_image"].copy(), "mask": None if mask.size == 0 else mask.copy(), "label": json.loads(str(z[k + "in_label"]))}
    pad = tuple(int(v) for v in z["pad"])
    crop_x, crop_y = (int(v) for v in z[k + "crop_xy"])
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=pad),
                  T.CropPad(pad=pad, center_perterb_max=int(z["center_perterb_max"]), crop_x=crop_x, crop_y=crop_y), T.Flip()]
    expected = {n: z[k + n] for n in ("image", "mask", "mask_small", "kpts", "objpos", "img_wh", "state")}
    return sample, transforms, int(z[k + "seed"]), expected


def label_arrays(label):
    people = [label] + list(label["processed_other_annotations"])
    return (np.array([p["keypoints"] for p in people], dtype=np.float64), np.array([p["objpos"] for p in people], dtype=np.float64),
            np.array([label["img_width"], label["img_height"]]))


def network_image(image_hwc):
    """coco.py:63-65: uint8 (H, W, 3) -> float32 (3, H, W) = (v - 128) / 256."""
    return ((image_hwc.astype(np.float32) - np.float32(128)) / np.float32(256)).transpose(2, 0, 1)


def synthetic_sample(seed, h, w, others=1, scale_provided=0.6, with_mask=True):
    g = np.random.default_rng(seed)

    def person():
        kps = [[float(g.uniform(0, w)), float(g.uniform(0, h)), int(g.integers(0, 2))] for _ in range(17)]
        return {"keypoints": kps, "objpos": [float(g.uniform(0.35, 0.65) * w), float(g.uniform(0.35, 0.65) * h)],
                "scale_provided": float(scale_provided)}
    label = person()
    label.update(img_width=w, img_height=h, processed_other_annotations=[person() for _ in range(others)])
    mask = None
    if with_mask:
        mask = np.ones((h, w), dtype=np.float32)
        mask[h // 4:h // 2, w // 3:w // 3 + max(w // 4, 1)] = 0
        mask[0, 0] = 0.5
    return {"image": g.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "mask": mask, "label": label}


def crop_sample(h, w, objpos, mask_value=1.0, seed=None):
    """A sample for CropPad alone: pixels in 0..99 (never a pad value used by the tests), 18 key-points, a constant mask."""
    g = np.random.default_rng(h * 100 + w if seed is None else seed)
    image = g.integers(0, 100, size=(h, w, 3), dtype=np.uint8)           # never the pad value
    label = {"keypoints": [[1.0, 2.0, 1] for _ in range(18)], "objpos": list(objpos), "img_width": w, "img_height": h,
             "processed_other_annotations": []}
    return {"image": image, "mask": np.full((h, w), mask_value, dtype=np.float32), "label": label}
