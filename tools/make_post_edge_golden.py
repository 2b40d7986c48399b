"""Generates tests/golden/post_edge_*.npz: the reference's own modules/keypoints.py (extract_keypoints + group_keypoints, demo
true and false) on the edge cases of tests/post_edge_cases.py.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_post_edge_golden.py

The reference needs up-sampled maps for the "maps" cases and cv2 is not installed: they are up-sampled with
oracle.post_ref.upsample_cubic, as oracle/make_golden.py does for the post_*.npz fixtures (the restated OpenCV cubic).
Only input digests, array shapes and the reference's outputs are written; the tests rebuild the inputs from the case
definitions.  Before a file is written every case's boundary statement (its ``expect``) is asserted through the oracle's
counts, and the oracle must equal the reference on it; two runs give identical files, each below 256 KiB.
"""
import io
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("LWP_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import post_edge_cases as pc  # noqa: E402

from modules import keypoints as ref_kp  # noqa: E402  (reference)

OUT = os.path.join(ROOT, "tests", "golden")


def save(kind, d):
    # np.savez_compressed stamps zip entries with the current time: write through a fixed-date ZipFile for identical files
    path = os.path.join(OUT, "post_edge_%s.npz" % kind)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(d[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    assert os.path.getsize(path) < 256 * 1024, (path, os.path.getsize(path))
    return path


def gen():
    files = {"group": {}, "full": {}, "maps": {}}
    for name, case in pc.all_cases().items():
        kind = case["kind"]
        d = files[kind]
        d["digest:" + name] = np.array(pc.input_digest(case))
        unbound = case["expect"].get("raises") == "unbound"
        for tag, demo in (("demo", True), ("val", False)):
            key = "%s:%s" % (name, tag)
            if unbound:                      # the reference itself must fail here, and so must the oracle
                for mod, counts in ((ref_kp, False), (pc.post_ref, True)):
                    try:
                        pc.run_oracle(case, demo, mod, counts)
                    except UnboundLocalError:
                        continue
                    raise AssertionError("%s: %s did not raise UnboundLocalError" % (key, mod.__name__))
                d["unbound:" + key] = np.array(1)
                continue
            ref = pc.run_oracle(case, demo, ref_kp, with_counts=False)
            ora = pc.run_oracle(case, demo)
            pc.check_expect(case, ora)                                         # the boundary statement, or no file
            for k in ("kp", "entries", "allk"):
                assert ref[k].shape == ora[k].shape and np.array_equal(ref[k], ora[k]), (key, k)
            d["kp:" + key], d["ent:" + key], d["allk:" + key] = ref["kp"], ref["entries"], ref["allk"]
            d["ent_shape:" + key] = np.array(ref["entries"].shape)
            if kind == "full":
                assert np.array_equal(ref["heat_mut"], ora["heat_mut"], equal_nan=True), key
                if tag == "demo":                                              # (extract_keypoints does not depend on demo)
                    d["mut:" + name] = ref["heat_mut"]
            elif kind == "maps":
                assert np.array_equal(ref["heat_mut"], ora["heat_mut"], equal_nan=True), key
                d["mut_digest:" + name] = np.array(pc.digest(ref["heat_mut"]))
    return [save(kind, d) for kind, d in files.items()]


if __name__ == "__main__":
    t0 = time.time()
    for path in gen():
        print(os.path.basename(path), os.path.getsize(path))
    print("%.1f s" % (time.time() - t0))
