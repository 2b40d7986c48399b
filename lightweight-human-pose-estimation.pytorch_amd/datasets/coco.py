"""Drop-in for the target side of the reference's ``datasets.coco`` (reference: datasets/coco.py:13-14, 48-61, 71-159): the
key-point and PAF target maps and the down-sampled mask of ``CocoTrainDataset.__getitem__``, rendered on the GPU for a whole
batch by ``lwp_train_targets`` / ``lwp_mask_downsample`` instead of the per-pixel Python loops of ``_add_gaussian`` /
``_set_paf``.  Together with ``get_mask`` below (reference: datasets/coco.py:17-21, 38-39) and ``datasets.transformations`` this
covers ``__getitem__`` from the mask on.

``get_mask`` is the reference's function in NumPy, the CPU path: it zeroes the crowd regions of a float mask from the
``segmentations`` of a label, which ``scripts/prepare_train_labels.py`` collects from ``iscrowd`` annotations.  In scope is what
COCO stores there, the uncompressed RLE dict ``{"counts": [c0, c1, ..], "size": [h, w]}``; a compressed ``counts`` string, a
polygon or a box is a ValueError.  On the GPU the same masks come from ``Engine.crowd_masks`` (``pack_crowd_runs`` makes the
arrays of the C call), and a sample of ``plan_batch`` / ``DeviceAugment`` / ``val.augmented_train_step`` may carry
``"segmentations"`` instead of a float ``"mask"``: the mask is then rendered on the device and never crosses PCIe.  Both restate
``maskApi.c``'s ``rleDecode`` and are unpinned against pycocotools itself.

Images are read by ``imread`` / ``CocoTrainDataset`` / ``CocoValDataset`` at the end of this file: baseline JPEG files, the
Huffman data decoded on the host and everything behind it on the GPU (``Engine.decode_jpeg_batch``), pinned against
libjpeg-turbo and not against ``cv2.imread`` itself.  Out of scope: reading annotations (``pycocotools``).  Labels arrive in
``scripts/prepare_train_labels.py``'s format, as ``datasets.transformations`` (the augmentations, host classes and the device
batch path) leaves them; ``generate_targets`` takes the float mask mean, ``val.augmented_train_step`` the reference's rounded
uint8 mask.
"""
import numbers
import os
import re

import numpy as np

BODY_PARTS_KPT_IDS = [[1, 8], [8, 9], [9, 10], [1, 11], [11, 12], [12, 13], [1, 2], [2, 3], [3, 4], [2, 16],
                      [1, 5], [5, 6], [6, 7], [5, 17], [1, 0], [0, 14], [0, 15], [14, 16], [15, 17]]


def _rle_counts(segmentation, h, w, where):
    """The counts of one uncompressed RLE dict as an int64 array, checked against an ``h`` x ``w`` image.  ``where`` names the
    sample in the ValueError."""
    if not isinstance(segmentation, dict) or "counts" not in segmentation or "size" not in segmentation:
        raise ValueError("%s: expected an uncompressed RLE dict {'counts': [...], 'size': [h, w]}, got %s (polygons and boxes are "
                         "out of scope)" % (where, type(segmentation).__name__))
    counts = segmentation["counts"]
    if isinstance(counts, (str, bytes)):
        raise ValueError("%s: compressed RLE counts (a string) are out of scope" % where)
    size = list(segmentation["size"])
    if size != [h, w]:
        raise ValueError("%s: an RLE of size %s does not belong to a %d x %d image" % (where, size, h, w))
    try:
        arr = np.asarray(counts)
    except (ValueError, OverflowError):
        arr = None
    if arr is not None and arr.size == 0:
        return np.zeros(0, dtype=np.int64)
    if arr is None or arr.ndim != 1 or arr.dtype.kind not in "iu":       # find the value to name
        for c in counts:
            if isinstance(c, bool) or not isinstance(c, (numbers.Integral, np.integer)):
                raise ValueError("%s: the count %r is not an integer" % (where, c))
        arr = np.asarray([int(c) for c in counts], dtype=object)
    if (arr < 0).any():
        raise ValueError("%s: the count %r is negative" % (where, arr[arr < 0][0]))
    total = int(arr.sum(dtype=object)) if arr.dtype != object else int(arr.sum())
    if total > h * w:
        raise ValueError("%s: the counts sum to %d, more than %d x %d" % (where, total, h, w))
    return arr.astype(np.int64)


def get_mask(segmentations, mask):
    """coco.py:17-21: zeroes, in place, the pixels of ``mask`` (H, W) that any of the RLE dicts covers, and returns ``mask``.
    The runs alternate between zeros and ones, start with zeros and walk the image column by column; what lies past the last
    run is zeros.  Nothing is written when a segmentation is refused."""
    h, w = int(mask.shape[0]), int(mask.shape[1])
    runs = [_rle_counts(seg, h, w, "segmentation %d" % k) for k, seg in enumerate(segmentations)]
    for counts in runs:
        flat = np.zeros(h * w, dtype=bool)
        flat[:int(counts.sum())] = np.repeat(np.arange(len(counts)) & 1, counts).astype(bool)
        mask[flat.reshape(w, h).T] = 0
    return mask


def pack_crowd_runs(segmentations_per_image, sizes):
    """The three host arrays of ``lwp_crowd_masks`` / ``lwp_augment_batch_crowd`` for a batch: ``counts`` (all counts, back to
    back), ``seg_off`` (S + 1) and ``image_seg_off`` (N + 1), int64.  ``segmentations_per_image``: per image a list of RLE dicts
    (``None`` counts as empty); ``sizes``: per image (height, width).  Raises the ValueErrors of ``get_mask``, naming the
    sample."""
    if len(segmentations_per_image) != len(sizes):
        raise ValueError("%d lists of segmentations for %d sizes" % (len(segmentations_per_image), len(sizes)))
    counts, seg_off, image_seg_off = [], [0], [0]
    for n, (segs, (h, w)) in enumerate(zip(segmentations_per_image, sizes)):
        for k, seg in enumerate(segs or []):
            counts.append(_rle_counts(seg, int(h), int(w), "sample %d, segmentation %d" % (n, k)))
            seg_off.append(seg_off[-1] + len(counts[-1]))
        image_seg_off.append(len(seg_off) - 1)
    flat = np.concatenate(counts) if counts else np.zeros(0, dtype=np.int64)
    return flat.astype(np.int64), np.asarray(seg_off, dtype=np.int64), np.asarray(image_seg_off, dtype=np.int64)


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


# ---------------------------------------------------------------------------------------------- reading the files
def _file_bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes), "<bytes>"
    with open(path_or_bytes, "rb") as f:
        return f.read(), str(path_or_bytes)


def imread(path_or_bytes, engine, entropy="host"):
    """``cv2.imread(path, cv2.IMREAD_COLOR)`` for a baseline JPEG file, decoded by ``Engine.decode_jpeg_batch``: a cuda uint8
    (H, W, 3) BGR tensor.  In scope: baseline (SOF0) files, grey or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan;
    progressive, arithmetic-coded, 12-bit and CMYK files, and every malformed one, are a ValueError that names the file and the
    reason.  The arithmetic is libjpeg's default integer path, pinned bit for bit against libjpeg-turbo as Pillow bundles it and
    NOT against cv2 itself.  The Exif orientation is not applied (``Engine.jpeg_info`` reports it), unlike
    ``cv2.imread`` from OpenCV 3.1 on.  ``entropy``: ``"host"`` (the default) or ``"device"``, where the Huffman data is decoded
    (DESIGN §3p); the pixels and the refusals are the same."""
    data, name = _file_bytes(path_or_bytes)
    try:
        return engine.decode_jpeg_batch([data], entropy=entropy)[0]
    except ValueError as e:
        raise ValueError("%s: %s" % (name, re.sub(r"^image 0: ", "", str(e)))) from None


def imwrite(path, img, engine, quality=95, subsampling="4:2:0"):
    """``cv2.imwrite(path, img)`` for a ``.jpg`` / ``.jpeg`` path: ``img`` (a uint8 (H, W, 3) BGR array or cuda tensor) is
    encoded by ``Engine.encode_jpeg_batch`` on the GPU and the file written.  The defaults are ``cv2.imwrite``'s for JPEG
    (quality 95, 4:2:0).  The arithmetic is libjpeg's default compression path, pinned byte for byte against the files Pillow
    (libjpeg-turbo) writes and NOT against cv2 itself, which is absent here.  Baseline files with Annex K's Huffman
    tables only: no grey, progressive or optimised output.  Returns True, as ``cv2.imwrite`` does; any other extension is a
    ValueError, an unwritable path an OSError."""
    if os.path.splitext(str(path))[1].lower() not in (".jpg", ".jpeg", ".jpe"):
        raise ValueError("%s: imwrite writes JPEG files (.jpg / .jpeg / .jpe) only" % (path,))
    engine = getattr(engine, "engine", engine)
    data = engine.encode_jpeg_batch([img], quality=quality, subsampling=subsampling)[0]
    with open(path, "wb") as f:
        f.write(data)
    return True


class _JpegFolder(object):
    """What the two datasets share: the folder, the engine, and the optional ``fallback(path) -> uint8 HxWx3 BGR`` for files
    the decoder refuses (``fallbacks`` counts its calls).  The package imports no decoder of its own accord.  ``entropy``:
    ``"host"`` (the default) or ``"device"``, passed to ``Engine.decode_jpeg_batch``."""

    def __init__(self, images_folder, engine, fallback=None, entropy="host"):
        self._entropy = entropy
        self._images_folder = images_folder
        self._engine = getattr(engine, "engine", engine)
        self._fallback = fallback
        self.fallbacks = 0

    def _read_batch(self, file_names):
        """The images of ``file_names`` as cuda uint8 (H, W, 3) tensors: every file the decoder takes in ONE device call."""
        import torch
        eng = self._engine
        paths = [os.path.join(self._images_folder, f) for f in file_names]
        images, datas = [None] * len(paths), []
        for path in paths:
            with open(path, "rb") as f:
                datas.append(f.read())
        todo = list(range(len(paths)))
        while todo:
            try:
                for i, img in zip(todo, eng.decode_jpeg_batch([datas[i] for i in todo], entropy=self._entropy)):
                    images[i] = img
                break
            except ValueError as e:                    # "image k: reason", k indexing this call's list; nothing was written
                m = re.match(r"image (\d+): (.*)", str(e), re.S)
                if m is None:
                    raise
                k = int(m.group(1))
                if self._fallback is None:
                    raise ValueError("%s: %s" % (paths[todo[k]], m.group(2))) from None
                del todo[k]                            # the fallback takes it below; the others are decoded again, without it
        for i, path in enumerate(paths):
            if images[i] is None:
                a = np.ascontiguousarray(self._fallback(path))
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                    raise ValueError("%s: the fallback must return a uint8 (H, W, 3) BGR array" % path)
                self.fallbacks += 1
                images[i] = torch.from_numpy(a).to(torch.device("cuda", eng.device_id))
        return images


class CocoValDataset(_JpegFolder):
    """The validation images of a COCO ground-truth file (reference: datasets/coco.py:162-178), for ``val.evaluate``: iterable
    and indexable, one ``{'file_name', 'img'}`` per entry of ``labels['images']`` with ``img`` a cuda uint8 (H, W, 3) BGR
    tensor.  ``labels``: the file's path or the dict."""

    def __init__(self, labels, images_folder, engine, fallback=None, entropy="host"):
        super().__init__(images_folder, engine, fallback, entropy)
        if isinstance(labels, dict):
            self._labels = labels
        else:
            import json
            with open(labels) as f:
                self._labels = json.load(f)

    def __len__(self):
        return len(self._labels["images"])

    def __getitem__(self, idx):
        file_name = self._labels["images"][idx]["file_name"]
        return {"file_name": file_name, "img": self._read_batch([file_name])[0]}

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class CocoTrainDataset(_JpegFolder):
    """The training samples of ``scripts/prepare_train_labels.py``'s label list (reference: datasets/coco.py:24-44) up to the
    transform: ``samples(indices)`` decodes the images of a batch in ONE device call and returns the dicts ``DeviceAugment`` /
    ``val.augmented_train_step`` take, ``'image'`` a cuda uint8 tensor the augment kernel reads in place, ``'label'`` a deep copy
    and ``'segmentations'`` the label's crowd RLEs (the mask is rendered on the device).  ``labels``: the pickle's path or the
    list itself."""

    def __init__(self, labels, images_folder, engine, fallback=None, entropy="host"):
        super().__init__(images_folder, engine, fallback, entropy)
        if isinstance(labels, (list, tuple)):
            self._labels = list(labels)
        else:
            import pickle
            with open(labels, "rb") as f:
                self._labels = pickle.load(f)

    def __len__(self):
        return len(self._labels)

    def samples(self, indices):
        import copy
        labels = [copy.deepcopy(self._labels[i]) for i in indices]
        images = self._read_batch([label["img_paths"] for label in labels])
        for label, image in zip(labels, images):
            if (int(image.shape[0]), int(image.shape[1])) != (label["img_height"], label["img_width"]):
                raise ValueError("%s is %d x %d but its label says %d x %d" % (label["img_paths"], image.shape[1], image.shape[0],
                                                                             label["img_width"], label["img_height"]))
        return [{"image": image, "label": label, "segmentations": label.get("segmentations", [])} for label, image in zip(labels, images)]

    def __getitem__(self, idx):
        return self.samples([idx])[0]
