"""Drop-in for the reference's ``scripts/prepare_train_labels.py``: COCO person key-point annotations -> the list of training
labels that ``datasets.transformations`` and ``datasets.coco`` consume, one label per person a crop is centred on.

    python -m lwpose_amd.scripts.prepare_train_labels --labels person_keypoints_train2017.json

``prepare(data, net_input_size)`` is the script's body for a loaded annotation file; ``prepare_annotations`` keeps the
reference's signature.  A label's ``segmentations`` are the image's ``iscrowd`` segmentations, COCO's uncompressed RLE dicts:
what ``datasets.coco.get_mask`` decodes and ``Engine.crowd_masks`` / ``Engine.augment_batch`` render on the device.  Host code
only; pinned to what the reference's own script returns (tests/golden/prepare_train_labels.json)."""
import argparse
import json
import pickle

MIN_KEYPOINTS, MIN_AREA = 5, 32 * 32
CLOSE_FRACTION = 0.3                                   # of the earlier person's box width


def _centre(bbox):
    return [bbox[0] + bbox[2] / 2, bbox[1] + bbox[3] / 2]


def _keypoints(flat):
    """COCO's flat [x, y, v, ..] -> rows [x, y, visibility] in the training convention: COCO's 1 (labelled, hidden) becomes 0,
    its 2 (visible) becomes 1, anything else 2 (absent)."""
    remap = {1: 0, 2: 1}
    return [[flat[3 * i], flat[3 * i + 1], remap.get(flat[3 * i + 2], 2)] for i in range(len(flat) // 3)]


def _person(annotation, net_input_size):
    return {"objpos": _centre(annotation["bbox"]), "bbox": annotation["bbox"], "segment_area": annotation["area"],
            "scale_provided": annotation["bbox"][3] / net_input_size, "num_keypoints": annotation["num_keypoints"],
            "keypoints": _keypoints(annotation["keypoints"])}


def prepare_annotations(annotations_per_image, images_info, net_input_size):
    """``annotations_per_image``: image id -> [person annotations, crowd segmentations].  A person gets a label when it has at
    least 5 key-points and 32 x 32 of area and its box centre is not within 0.3 box widths of a person of the image that
    already has one; every OTHER annotation of the image (compared by value, as the reference does) rides along in
    ``processed_other_annotations``, the small and the close ones included."""
    prepared = []
    for people, segmentations in annotations_per_image.values():
        kept = []                                      # (centre x, centre y, box width) of the persons labelled so far
        for annotation in people:
            if annotation["num_keypoints"] < MIN_KEYPOINTS or annotation["area"] < MIN_AREA:
                continue
            cx, cy = _centre(annotation["bbox"])
            if any(((cx - px) ** 2 + (cy - py) ** 2) ** 0.5 < pw * CLOSE_FRACTION for px, py, pw in kept):
                continue
            info = images_info[annotation["image_id"]]
            label = _person(annotation, net_input_size)
            label.update(img_paths=info["file_name"], img_width=info["width"], img_height=info["height"],
                         image_id=annotation["image_id"], segmentations=segmentations,
                         processed_other_annotations=[_person(other, net_input_size) for other in people if other != annotation])
            prepared.append(label)
            kept.append((cx, cy, annotation["bbox"][2]))
    return prepared


def prepare(data, net_input_size=368):
    """A loaded COCO key-point annotation file -> the labels.  Persons: annotations with key-points that are not crowds, by
    image in order of first appearance.  Crowd segmentations reach the images that have persons; a crowd on an image without
    any is dropped with the image."""
    per_image = {}
    for annotation in data["annotations"]:
        if annotation["num_keypoints"] != 0 and not annotation["iscrowd"]:
            per_image.setdefault(annotation["image_id"], [[], []])[0].append(annotation)
    for annotation in data["annotations"]:
        if annotation["iscrowd"] and annotation["image_id"] in per_image:
            per_image[annotation["image_id"]][1].append(annotation["segmentation"])
    images_info = {info["id"]: info for info in data["images"]}
    return prepare_annotations(per_image, images_info, net_input_size)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--labels", type=str, required=True, help="COCO person key-point annotations (json)")
    parser.add_argument("--output-name", type=str, default="prepared_train_annotation.pkl",
                        help="pickle file the labels are written to")
    parser.add_argument("--net-input-size", type=int, default=368, help="side of the training crop: scale_provided is box height over it")
    args = parser.parse_args()
    with open(args.labels, "r") as f:
        labels = prepare(json.load(f), args.net_input_size)
    with open(args.output_name, "wb") as f:
        pickle.dump(labels, f)
