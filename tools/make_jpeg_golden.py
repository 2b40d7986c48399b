"""Writes the JPEG fixtures of tests/golden: small files made with Pillow and Pillow's own decode of each (libjpeg-turbo's
default path: slow-but-accurate integer IDCT, fancy up-sampling, table-driven colour conversion), which is what the tests hold
the restatement (tests/jpeg_cases.py) and the library to, byte for byte.  Needs Pillow; the tests do not.

    python tools/make_jpeg_golden.py [--extra some_baseline.jpg]

``--extra`` adds a file from elsewhere (a real camera / encoder file) as tests/golden/jpeg_extra.npz: its bytes, a 256 x 256
window of Pillow's pixels at an origin that is no multiple of 8, and the CRC32 of all of them.

Every fixture is checked with the restatement before it is written: it must equal Pillow in every byte, and no inverse-DCT output
may leave [-512, 511] before the + 128 (beyond that libjpeg's masked range-limit table wraps where this project clamps).
"""
import argparse
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases  # noqa: E402

SAMPLING = {"444": 0, "422": 1, "420": 2}            # Pillow's subsampling argument
SIZES = [(1, 1), (8, 8), (16, 16), (17, 17), (9, 31), (33, 16), (16, 33), (37, 53)]          # (width, height)
# stage A takes 32 blocks a workgroup and stage B 1024 pixels (256 threads x 4): 100 x 75 at 4:2:0 is 140 + 35 + 35 blocks and
# 1875 pixel groups, several workgroups in both stages on its own; neither kernel has a grid-stride loop
LARGE = (100, 75)


def smooth(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        a, b, p = rng.uniform(0.05, 0.6, 3)
        img[:, :, c] = 128 + 100 * np.sin(a * x + p * 6) * np.cos(b * y + c) + rng.normal(0, 6, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def one_bit(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def encode(arr, **kw):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pillow_pixels(data):
    im = Image.open(io.BytesIO(data))
    assert im.mode in ("RGB", "L"), im.mode
    return np.asarray(im)


def cases():
    out = {}
    seed = 0
    for w, h in SIZES:
        for name, sub in SAMPLING.items():
            seed += 1
            out["%dx%d_%s" % (w, h, name)] = encode(smooth(w, h, seed), quality=85, subsampling=sub)
    out["grey_19x21"] = encode(smooth(19, 21, 100)[:, :, 0], quality=80)
    out["optimised_37x53_420"] = encode(smooth(37, 53, 101), quality=75, subsampling=2, optimize=True)
    out["optimised_33x16_444"] = encode(noise(33, 16, 102), quality=60, subsampling=0, optimize=True)
    out["restart2_37x53_420"] = encode(smooth(37, 53, 103), quality=85, subsampling=2, restart_marker_blocks=2)
    out["restart2_33x16_422"] = encode(noise(33, 16, 104), quality=70, subsampling=1, restart_marker_blocks=2)
    out["onebit_q30_40x24_420"] = encode(one_bit(40, 24, 105), quality=30, subsampling=2)
    out["onebit_q30_17x17_444"] = encode(one_bit(17, 17, 106), quality=30, subsampling=0)
    out["onebit_q30_33x16_422"] = encode(one_bit(33, 16, 107), quality=30, subsampling=1)
    out["noise_q95_24x24_444"] = encode(noise(24, 24, 108), quality=95, subsampling=0)
    out["noise_q95_37x53_420"] = encode(noise(37, 53, 109), quality=95, subsampling=2)
    out["large_%dx%d_420" % LARGE] = encode(smooth(LARGE[0], LARGE[1], 110), quality=90, subsampling=2)
    exif = Image.Exif()
    exif[0x0112] = 6
    out["exif6_16x16_420"] = encode(smooth(16, 16, 111), quality=85, subsampling=2, exif=exif.tobytes())
    # 0xFF fill bytes in front of markers: legal anywhere a marker stands (ITU T.81 B.1.1.2)
    d = out["restart2_33x16_422"]
    d = d.replace(b"\xff\xda", b"\xff\xff\xff\xda", 1)
    for n in range(8):
        d = d.replace(bytes([0xFF, 0xD0 + n]), bytes([0xFF, 0xFF, 0xD0 + n]))
    out["fill_bytes_33x16_422"] = d
    # a single-component file whose frame header states 2x2 sampling: still one block per MCU
    g = bytearray(out["grey_19x21"])
    sof = g.index(b"\xff\xc0")
    assert g[sof + 9] == 1 and g[sof + 11] == 0x11
    g[sof + 11] = 0x22
    out["grey_2x2_19x21"] = bytes(g)
    return out


def check(name, data, rgb):
    img, (lo, hi) = jpeg_cases.decode_bgr(data, want_range=True)
    ref = rgb[:, :, ::-1] if rgb.ndim == 3 else np.repeat(rgb[:, :, None], 3, axis=2)
    diff = int((img != ref).sum())
    assert diff == 0, "%s: the restatement differs from Pillow in %d bytes" % (name, diff)
    assert -512 <= lo and hi <= 511, "%s: IDCT output %d..%d leaves [-512, 511]" % (name, lo, hi)
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extra")
    args = ap.parse_args()
    arrays, lo, hi = {}, 0, 0
    for name, data in cases().items():
        rgb = pillow_pixels(data)
        l, h = check(name, data, rgb)
        lo, hi = min(lo, l), max(hi, h)
        arrays["jpeg/" + name] = np.frombuffer(data, dtype=np.uint8)
        arrays["rgb/" + name] = rgb
    path = os.path.join(jpeg_cases.GOLDEN, "jpeg_cases.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d files, %d bytes, IDCT output within [%d, %d]" % (path, len(arrays) // 2, os.path.getsize(path), lo, hi))
    if args.extra:
        data = open(args.extra, "rb").read()
        rgb = pillow_pixels(data)
        l, h = check("extra", data, rgb)
        oy, ox = 101, 203
        assert rgb.ndim == 3 and rgb.shape[0] >= oy + 256 and rgb.shape[1] >= ox + 256
        path = os.path.join(jpeg_cases.GOLDEN, "jpeg_extra.npz")
        np.savez_compressed(path, jpeg=np.frombuffer(data, dtype=np.uint8), window=rgb[oy:oy + 256, ox:ox + 256],
                            origin=np.array([oy, ox]), shape=np.array(rgb.shape), crc32=np.array([zlib.crc32(rgb.tobytes())], dtype=np.uint64))
        print("%s: %d bytes, IDCT output within [%d, %d]" % (path, os.path.getsize(path), l, h))


if __name__ == "__main__":
    main()
