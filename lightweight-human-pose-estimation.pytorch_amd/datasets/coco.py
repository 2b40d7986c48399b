"""Drop-in for the target side of the reference's ``datasets.coco`` (reference: datasets/coco.py:13-14, 48-61, 71-159): the
key-point and PAF target maps and the down-sampled mask of ``CocoTrainDataset.__getitem__``, rendered on the GPU for a whole
batch by ``lwp_train_targets`` / ``lwp_mask_downsample`` instead of the per-pixel Python loops of ``_add_gaussian`` /
``_set_paf``.

Out of scope: reading images and annotations (``cv2.imread``, ``pycocotools``) and ``get_mask``.  Labels arrive in
``scripts/prepare_train_labels.py``'s format, as ``datasets.transformations`` (the augmentations, host classes and the device
batch path) leaves them; ``generate_targets`` takes the float mask mean, ``val.augmented_train_step`` the reference's rounded
uint8 mask.
"""
import numpy as np

BODY_PARTS_KPT_IDS = [[1, 8], [8, 9], [9, 10], [1, 11], [11, 12], [12, 13], [1, 2], [2, 3], [3, 4], [2, 16],
                      [1, 5], [5, 6], [6, 7], [5, 17], [1, 0], [0, 14], [0, 15], [14, 16], [15, 17]]


def labels_to_arrays(labels, K=18):
    """Label dicts (``keypoints``: K rows [x, y, visibility]; ``processed_other_annotations``: a list of dicts with their own
    ``keypoints``) -> (kpts (N, Pmax, K, 3) float64, n_persons (N,) int32).  Row 0 of a frame is the main person, the others
    follow in list order: the order in which the reference adds Gaussians and overwrites PAFs.  Unused rows hold visibility 2."""
    people = []
    for label in labels:
        rows = [label["keypoints"]] + [other["keypoints"] for other in label.get("processed_other_annotations", [])]
        rows = [np.asarray(r, dtype=np.float64).reshape(-1, 3) for r in rows]
        for r in rows:
            if r.shape != (K, 3):
                raise ValueError("a person has %d key-points, expected %d" % (r.shape[0], K))
        people.append(rows)
    n = np.array([len(p) for p in people], dtype=np.int32)
    kpts = np.zeros((len(people), int(n.max()) if len(n) else 0, K, 3), dtype=np.float64)
    kpts[..., 2] = 2.0
    for f, rows in enumerate(people):
        for i, r in enumerate(rows):
            kpts[f, i] = r
    return kpts, n


def generate_targets(net, labels, image_hw, mask=None, stride=8, sigma=7, paf_thickness=1):
    """The target half of ``CocoTrainDataset.__getitem__`` (coco.py:48-61) for a batch of same-sized frames.  ``net``: a
    ``PoseEstimationWithMobileNet`` (or an ``Engine``) whose skeleton fixes K and the limb table; ``labels``: one dict per
    frame; ``image_hw``: (H, W) of the transformed frames; ``mask``: (N, H, W) float32 (1 = counts, as ``get_mask`` makes it;
    H and W multiples of the stride) or None for all ones.  Returns float32 cuda tensors ``keypoint_maps`` (N, K + 1, h, w),
    ``paf_maps`` (N, 2L, h, w) and ``keypoint_mask`` / ``paf_mask``, which are broadcast VIEWS of one (N, h, w) mask (the
    reference copies it into every channel)."""
    import torch
    eng = getattr(net, "engine", net)
    K = eng.skeleton["num_kpt_types"]
    kpts, n_persons = labels_to_arrays(labels, K)
    kmaps, pmaps = eng.train_targets(kpts, n_persons, image_hw, stride, sigma, paf_thickness)
    if mask is None:
        small = torch.ones((kmaps.shape[0],) + tuple(kmaps.shape[2:]), dtype=torch.float32, device=kmaps.device)
    else:
        small = eng.mask_downsample(mask, stride)
        if tuple(small.shape) != (kmaps.shape[0],) + tuple(kmaps.shape[2:]):
            raise ValueError("mask of shape %s does not belong to %d frames of %s" % (tuple(mask.shape), kmaps.shape[0], tuple(image_hw)))
    return {"keypoint_maps": kmaps, "paf_maps": pmaps,
            "keypoint_mask": small[:, None].expand(-1, kmaps.shape[1], -1, -1),
            "paf_mask": small[:, None].expand(-1, pmaps.shape[1], -1, -1)}
