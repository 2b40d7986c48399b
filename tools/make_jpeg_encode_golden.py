"""Writes the JPEG ENCODE fixtures of tests/golden/encjpeg_edges.npz (and, with ``--cases``, of encjpeg_cases.npz and
encjpeg_tables.npz, which are otherwise left as they are): small BGR frames and the file Pillow (libjpeg-turbo's
default compression path: 16-bit fixed-point colour conversion, h2v1 / h2v2 box down-sampling, slow-but-accurate integer forward
DCT, Annex K's Huffman tables) writes of each, which is what the tests hold the restatement (tests/jpeg_encode_cases.py) and the
library to, byte for byte.  Needs Pillow; the tests do not.

    python tools/make_jpeg_encode_golden.py [--cases]

Every fixture is checked before it is written: the restatement must give the coefficients jpeg_cases.decode_blocks reads from
Pillow's file, none differing.  The table of all hundred qualities (tests/golden/encjpeg_tables.npz) is read from Pillow's files
too.
"""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases  # noqa: E402
import jpeg_encode_cases as jen  # noqa: E402

# (width, height): both bottom-padding rules (H = 8, 24, 40 at 4:2:0), dummy blocks to the right (W = 17, 23, 50 -> an odd number
# of luma block columns) and below, partial MCUs both ways
SIZES = [(1, 1), (7, 7), (9, 8), (32, 16), (23, 17), (17, 24), (25, 24), (9, 40), (50, 33), (65, 31), (75, 100)]
QUALITIES = [1, 30, 75, 95, 100]                    # all-255 tables, long codes, all-ones tables
# the long case: 13 x 10 x 3 = 390 blocks (more than one 256-block workgroup of the length and write passes, more than one
# 256-block tile of the offset scan) and some 25 KB of scan (more than one 8192-byte tile of the stuffing passes)
LONG = (100, 75)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        a, b, p = rng.uniform(0.05, 0.6, 3)
        img[:, :, c] = 128 + 100 * np.sin(a * x + p * 6) * np.cos(b * y + c) + rng.normal(0, 6, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def checker(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def pillow_file(bgr, quality, sampling, restart):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling=jen.PILLOW[sampling],
                                                                 restart_marker_blocks=restart)
    return buf.getvalue()


def cases():
    """{name: (bgr, quality, sampling, restart interval in MCUs)}"""
    out, seed = {}, 0
    for w, h in SIZES:
        for sampling in jen.SAMPLINGS:
            q = QUALITIES[seed % len(QUALITIES)]
            seed += 1
            out["noise_%dx%d_%s_q%d" % (w, h, jen.SHORT[sampling], q)] = (noise(w, h, seed), q, sampling, 0)
    for k, sampling in enumerate(jen.SAMPLINGS):
        s = jen.SHORT[sampling]
        mcus_x = -(-50 // (8 * jen.SAMPLINGS[sampling][0]))
        out["restart1_50x33_%s" % s] = (noise(50, 33, 200 + k), 75, sampling, 1)
        out["restartrow_50x33_%s" % s] = (smooth(50, 33, 210 + k), 95, sampling, mcus_x)
        out["restartbig_23x17_%s" % s] = (noise(23, 17, 220 + k), 30, sampling, 1000)
        out["restart1_many_65x31_%s" % s] = (smooth(65, 31, 230 + k), 75, sampling, 1)        # more than 8 intervals: RST7 -> RST0
        out["smooth_65x31_%s" % s] = (smooth(65, 31, 240 + k), 75, sampling, 0)
        out["zeros_17x24_%s" % s] = (np.zeros((24, 17, 3), dtype=np.uint8), 75, sampling, 0)
        out["ones_25x24_%s" % s] = (np.full((24, 25, 3), 255, dtype=np.uint8), 95, sampling, 0)
        out["checker_23x17_%s" % s] = (checker(23, 17), 100, sampling, 0)
    out["long_%dx%d_444_q100" % LONG] = (noise(LONG[0], LONG[1], 300), 100, "4:4:4", 0)
    out["long_restart3_%dx%d_444_q100" % LONG] = (noise(LONG[0], LONG[1], 301), 100, "4:4:4", 3)
    return out


TILE_COLOURS = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 255), (0, 0, 255), (255, 255, 0)]      # BGR: black, white, blue, yellow, red, cyan


def tiles(w, h):
    """16 x 16 tiles of saturated colours in turn: at quality 100 the DC steps between neighbouring blocks of all three
    components reach the categories 10 and 11."""
    y, x = np.mgrid[0:h, 0:w]
    index = ((y // 16) * -(-w // 16) + x // 16) % len(TILE_COLOURS)
    return np.array(TILE_COLOURS, dtype=np.uint8)[index]


def edge_cases():
    """What stages B .. F of the encoder see too rarely from the cases above: DC categories 10 and 11 in both tables, and a
    restart interval that starts on the first lane of the offset scan's second tile (4:2:2, 144 x 64, restart 1: 72 intervals
    of 4 blocks, one of which starts at block 256).  144 x 64 comes in all three samplings, as every size but the long one does."""
    out = {}
    for k, sampling in enumerate(jen.SAMPLINGS):
        s = jen.SHORT[sampling]
        out["tiles_99x37_%s" % s] = (tiles(99, 37), 100, sampling, 0)
        out["seam_144x64_%s" % s] = (noise(144, 64, 400 + k), 75, sampling, 1)
    return out


def write(path, which):
    arrays, coefs, differing = {}, 0, 0
    for name, (bgr, quality, sampling, restart) in which.items():
        data = pillow_file(bgr, quality, sampling, restart)
        hd, want, qt = jpeg_cases.decode_blocks(data)
        g, got, qt_got = jen.forward_blocks(bgr, sampling, quality)
        assert hd["restart_interval"] == restart and got.shape == want.shape, name
        assert np.array_equal(qt, qt_got), name
        d = int((got != want).sum())
        coefs += want.size
        differing += d
        assert d == 0, "%s: the restatement differs from Pillow in %d coefficients" % (name, d)
        arrays["jpeg/" + name] = np.frombuffer(data, dtype=np.uint8)
        arrays["bgr/" + name] = bgr
        arrays["opts/" + name] = np.array([quality, jen.PILLOW[sampling], restart], dtype=np.int32)
    np.savez_compressed(path, **arrays)
    print("%s: %d files, %d bytes; %d of %d coefficients differ" % (path, len(arrays) // 3, os.path.getsize(path), differing, coefs))


def main():
    write(os.path.join(jpeg_cases.GOLDEN, "encjpeg_edges.npz"), edge_cases())
    if "--cases" not in sys.argv[1:]:
        return
    write(os.path.join(jpeg_cases.GOLDEN, "encjpeg_cases.npz"), cases())
    tables = np.zeros((100, 2, 64), dtype=np.uint16)
    for q in range(1, 101):
        _, _, qt = jpeg_cases.decode_blocks(pillow_file(noise(8, 8, q), q, "4:4:4", 0))
        tables[q - 1] = qt[:2]
    path = os.path.join(jpeg_cases.GOLDEN, "encjpeg_tables.npz")
    np.savez_compressed(path, tables=tables)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
