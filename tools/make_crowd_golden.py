"""Record tests/golden/prepare_train_labels.json from the REFERENCE's own scripts/prepare_train_labels.py.

    LWP_REFERENCE=/path/to/lightweight-human-pose-estimation.pytorch python tools/make_crowd_golden.py

The reference's script depends only on argparse, json and pickle, so it runs here as it is: it is executed unchanged as
``__main__`` on a synthetic annotation file (nothing of it is copied) and the pickle it writes is read back.  The fixture
holds the annotations and the list the script returned for them.  The annotations cover: people under 5 key-points, people
under 32 x 32 of area, two people with close centres, a person without key-points, a crowd annotation on an image with people
(two on another) and one on an image without, and an image without a crowd.  No GPU needed."""
import json
import os
import pickle
import random
import runpy
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "prepare_train_labels.json")
NET_INPUT_SIZE = 368


def person(g, ann_id, image_id, bbox, num_keypoints, area=None):
    kps = []
    for k in range(17):
        v = g.choice([1, 2]) if k < num_keypoints else 0
        kps += [round(g.uniform(bbox[0], bbox[0] + bbox[2]), 1), round(g.uniform(bbox[1], bbox[1] + bbox[3]), 1), v] if v else [0, 0, 0]
    return {"id": ann_id, "image_id": image_id, "category_id": 1, "iscrowd": 0, "bbox": bbox, "num_keypoints": num_keypoints,
            "area": bbox[2] * bbox[3] * 0.6 if area is None else area, "keypoints": kps}


def crowd(ann_id, image_id, counts, h, w):
    assert sum(counts) <= h * w
    return {"id": ann_id, "image_id": image_id, "category_id": 1, "iscrowd": 1, "bbox": [0, 0, 1, 1], "num_keypoints": 0, "area": 1.0,
            "keypoints": [0] * 51, "segmentation": {"counts": counts, "size": [h, w]}}


def annotations():
    g = random.Random(7)
    images = [{"id": 11, "file_name": "000000000011.jpg", "width": 64, "height": 48},
              {"id": 5, "file_name": "000000000005.jpg", "width": 40, "height": 30},
              {"id": 23, "file_name": "000000000023.jpg", "width": 52, "height": 36},
              {"id": 8, "file_name": "000000000008.jpg", "width": 33, "height": 57}]
    anns = [
        crowd(100, 11, [100, 40, 8, 40, 8, 40, 2000], 48, 64),                       # in front of its image's people
        person(g, 101, 11, [2.5, 4.0, 41.0, 40.5], 12, area=1500.5),
        person(g, 102, 11, [30.0, 3.0, 33.0, 44.0], 3),                              # under 5 key-points
        person(g, 103, 11, [40.0, 10.0, 20.0, 30.0], 9, area=900.0),                 # under 32 x 32
        person(g, 104, 11, [6.0, 5.5, 38.0, 39.0], 15, area=1400.0),                # centre within 0.3 widths of 101's
        person(g, 105, 11, [36.25, 1.0, 27.5, 46.0], 7, area=1024.0),                # far enough, exactly 32 x 32
        crowd(106, 5, [0, 30, 500], 30, 40),                                         # an image without people: dropped
        person(g, 107, 23, [1.0, 1.0, 50.0, 34.0], 17, area=1600.25),
        person(g, 108, 23, [10.0, 5.0, 30.0, 30.0], 0),                              # no key-points: never a person
        crowd(109, 23, [0, 36, 36, 36], 36, 52),
        crowd(110, 23, [700, 5, 31, 5, 31, 5], 36, 52),
        person(g, 111, 8, [0.0, 0.0, 33.0, 57.0], 5),                                # no crowd on its image
        person(g, 112, 8, [15.0, 27.0, 4.0, 6.0], 6),                                # too small, still an "other"
    ]
    return {"images": images, "annotations": anns, "categories": [{"id": 1, "name": "person"}]}


def run_reference(data):
    script = os.path.join(os.environ["LWP_REFERENCE"], "scripts", "prepare_train_labels.py")
    with tempfile.TemporaryDirectory() as tmp:
        labels, out = os.path.join(tmp, "labels.json"), os.path.join(tmp, "prepared.pkl")
        with open(labels, "w") as f:
            json.dump(data, f)
        argv = sys.argv
        sys.argv = [script, "--labels", labels, "--output-name", out, "--net-input-size", str(NET_INPUT_SIZE)]
        try:
            runpy.run_path(script, run_name="__main__")
        finally:
            sys.argv = argv
        with open(out, "rb") as f:
            return pickle.load(f)


def main():
    data = json.loads(json.dumps(annotations()))       # what the script will read back from the file
    expected = run_reference(data)
    assert len(expected) == 4 and [e["image_id"] for e in expected] == [11, 11, 23, 8], [e["image_id"] for e in expected]
    with open(OUT, "w") as f:
        json.dump({"net_input_size": NET_INPUT_SIZE, "data": data, "expected": expected}, f, indent=1)
    print("%s: %d labels from %d annotations" % (OUT, len(expected), len(data["annotations"])))


if __name__ == "__main__":
    main()
