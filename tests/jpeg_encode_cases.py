"""A NumPy restatement of the JPEG encoder's forward path (csrc/jpeg_encode_kernels.hip): libjpeg's default
compression path from BGR pixels to quantised coefficients in the project's layout (int16, natural order, plane order,
MCU-padded grids), the fixtures of tests/golden/encjpeg_*.npz (source pixels and the file Pillow wrote of them), and hand-built
AVI / Motion-JPEG containers for the reader.  The restatement is the oracle of test_jpeg_encode_host.py and
test_gpu_jpeg_encode.py; it is itself pinned against the coefficients jpeg_cases.decode_blocks reads from Pillow's files.

Mutation knobs (``mutant``) build deliberately wrong encoders: the tests use them to show that the fixtures would see a bottom
edge padded before the down-sampling, a right edge replicated instead of dummy blocks, a constant down-sampling bias and a
truncating quantiser."""
import glob
import os
import struct

import numpy as np

import jpeg_cases as jc
import jpeg_entropy_cases as jec

GOLDEN = jc.GOLDEN
SAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
SHORT = {"4:4:4": "444", "4:2:2": "422", "4:2:0": "420"}      # jpeg_entropy_cases' names
PILLOW = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}                 # Pillow's ``subsampling`` numbers (and the library's)
MUTANTS = ("bottom_before_downsample", "replicate_right", "constant_bias", "truncating_quantiser")

# ITU T.81 Annex K, tables K.1 and K.2, natural order
STD_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
            100, 103, 99]
STD_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
              99] + [99] * 32


def quality_tables(quality):
    """jpeg_quality_scaling and jpeg_add_quant_table with force_baseline: uint16 (4, 64), natural order, slots 0 and 1."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    qt = np.zeros((4, 64), dtype=np.uint16)
    for slot, std in enumerate((STD_LUMA, STD_CHROMA)):
        qt[slot] = np.clip((np.array(std, dtype=np.int64) * scale + 50) // 100, 1, 255)
    return qt


def geometry(width, height, sampling):
    """jpeg_entropy_cases.geometry and, as ``real_w`` / ``real_h``, each component's real blocks: ceil(ceil(W h / hmax) / 8)."""
    g = jec.geometry(width, height, SHORT[sampling])
    hs, vs = SAMPLINGS[sampling]
    g["real_w"] = [-(-(-(-width * h // hs)) // 8) for h in g["h_samp"]]
    g["real_h"] = [-(-(-(-height * v // vs)) // 8) for v in g["v_samp"]]
    return g


def _edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_planes(bgr, sampling, mutant=None):
    """The three sample planes, each real_h * 8 by real_w * 8 (with ``replicate_right``: the MCU-padded width), int64."""
    H, W = bgr.shape[:2]
    hs, vs = SAMPLINGS[sampling]
    g = geometry(W, H, sampling)
    b, gr, r = [bgr[:, :, k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16
    cols = [(g["blocks_w"] if mutant == "replicate_right" else g["real_w"])[c] * 8 for c in range(3)]
    rows = [g["real_h"][c] * 8 for c in range(3)]
    planes = [_edge(y, rows[0], cols[0])]
    for c, p in ((1, cb), (2, cr)):
        if mutant == "bottom_before_downsample":
            p = _edge(p, rows[c] * vs, cols[c] * hs)
        else:
            p = _edge(p, -(-H // vs) * vs, cols[c] * hs)               # the bottom: up to a multiple of vmax rows only
        if (hs, vs) == (2, 1):
            bias = np.arange(cols[c]) & 1
            if mutant == "constant_bias":
                bias = 1
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        elif (hs, vs) == (2, 2):
            bias = 1 + (np.arange(cols[c]) & 1)
            if mutant == "constant_bias":
                bias = 2
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        planes.append(_edge(p, rows[c], cols[c]))                      # then the down-sampled last row is repeated
    return planes


def _fdct8(x, axis, first):
    """jfdctint.c's 8-point pass along ``axis``: the row pass (``first``) leaves PASS1_BITS of scale, the column pass removes
    them; every DESCALE with its rounding term."""
    d = [np.take(x, k, axis=axis) for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2

    def descale(v, n):
        return (v + (1 << (n - 1))) >> n
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
        n = 11
    else:
        out[0], out[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
        n = 15
    z1 = (t12 + t13) * 4433
    out[2] = descale(z1 + t13 * 6270, n)
    out[6] = descale(z1 + t12 * -15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(out, axis=axis)


def forward_blocks(bgr, sampling, quality, mutant=None):
    """(geometry, coefficients int16 (total_blocks, 64), qtables uint16 (4, 64)) of a BGR uint8 (H, W, 3) frame, laid out as
    jpeg_cases.decode_blocks lays out what it reads from the file."""
    H, W = bgr.shape[:2]
    g = geometry(W, H, sampling)
    qt = quality_tables(quality)
    out = []
    for c, plane in enumerate(component_planes(bgr, sampling, mutant)):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blk = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)          # [block row][block column][row][column]
        blk = _fdct8(_fdct8(blk, 3, True), 2, False).reshape(bh, bw, 64)         # each row first, then each column
        q8 = 8 * qt[min(c, 1)].astype(np.int64)
        mag = np.abs(blk) // q8 if mutant == "truncating_quantiser" else (np.abs(blk) + (q8 >> 1)) // q8
        real = np.sign(blk) * mag
        grid = np.zeros((g["blocks_h"][c], g["blocks_w"][c], 64), dtype=np.int64)
        grid[:bh, :bw] = real
        hc, vc = g["h_samp"][c], g["v_samp"][c]
        for by in range(g["blocks_h"][c]):                                       # jccoefct.c's compress_data: dummy blocks
            for bx in range(g["blocks_w"][c]):
                if by < bh and bx < bw:
                    continue
                if by < bh:
                    grid[by, bx, 0] = grid[by, bx - 1, 0]                         # right of a real block: its left neighbour's DC
                else:
                    last = (bx // hc) * hc + hc - 1                               # the last block of the row above inside the MCU
                    grid[by, bx, 0] = grid[by - 1, last, 0]
            assert vc <= 2
        out.append(grid.reshape(-1, 64))
    return g, np.concatenate(out).astype(np.int16), qt


def scan_of(coef, g, restart_interval=0):
    """The entropy-coded scan of such coefficients with Annex K's Huffman tables: jpeg_entropy_cases' coder."""
    return jec.encode_scan(coef, g, jec.standard_tables(), [0, 1, 1], [0, 1, 1], restart_interval)


# ---------------------------------------------------------------------------------------------- fixtures
_FIXTURES = None


def fixtures():
    """{name: dict(bgr, jpeg, quality, sampling, restart)} of every tests/golden/encjpeg_*.npz, loaded once."""
    global _FIXTURES
    if _FIXTURES is None:
        out = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "encjpeg_*.npz"))):
            with np.load(path) as z:
                for name in [k[5:] for k in z.files if k.startswith("jpeg/")]:
                    quality, sampling, restart = [int(v) for v in z["opts/" + name]]
                    out[name] = {"bgr": np.ascontiguousarray(z["bgr/" + name]), "jpeg": z["jpeg/" + name].tobytes(), "quality": quality,
                                 "sampling": {v: k for k, v in PILLOW.items()}[sampling], "restart": restart}
        _FIXTURES = out
    return _FIXTURES


_RESTATED = {}


def restated(name):
    """(geometry, coefficients, qtables) of a fixture by the restatement, computed once per process."""
    if name not in _RESTATED:
        f = fixtures()[name]
        _RESTATED[name] = forward_blocks(f["bgr"], f["sampling"], f["quality"])
    return _RESTATED[name]


# ---------------------------------------------------------------------------------------------- containers, from their specification
def dht_segments():
    """Annex K's four tables as the DHT segments a full file carries (DC 0, AC 0, DC 1, AC 1)."""
    t = jec.standard_tables()
    out = b""
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        counts, vals = t[key]
        body = bytes([(key[0] << 4) | key[1]] + list(counts) + list(vals))
        out += b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    return out


def strip_dht(data):
    """The file without its DHT segments, as many cameras write their Motion-JPEG frames."""
    data = bytes(data)
    out, pos = bytearray(data[:2]), 2
    while True:
        m = data[pos + 1]
        L = int.from_bytes(data[pos + 2:pos + 4], "big")
        if m != 0xC4:
            out += data[pos:pos + 2 + L]
        pos += 2 + L
        if m == 0xDA:
            return bytes(out) + data[pos:]


def _chunk(fourcc, body):
    return fourcc + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _list(kind, body):
    return b"LIST" + struct.pack("<I", len(body) + 4) + kind + body


def build_avi(frames, width, height, fps=25, handler=b"MJPG", audio=True, rec=True, riff_kind=b"AVI ", video_stream=None):
    """A RIFF AVI written from the container's specification (not by VideoWriter): ``frames`` is a list of JPEG files, b""
    for a dropped frame.  With ``audio`` an ``auds`` stream comes FIRST in the header list (so the video stream is number 1 and
    its chunks are ``01dc``) and a ``00wb`` chunk of odd length stands between the frames; with ``rec`` the first two frames lie
    in a ``LIST rec ``; a JUNK chunk stands in front of the second half.  No idx1: a reader walks ``movi``."""
    vid = 1 if audio else 0
    if video_stream is not None:
        vid = video_stream
    tag = b"%02ddc" % vid
    avih = struct.pack("<14I", 1000000 // fps, 0, 0, 0x10, len(frames), 0, 2 if audio else 1, 0, width, height, 0, 0, 0, 0)
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", handler, 0, 0, 0, 0, 1, fps, 0, len(frames), 0, 0xFFFFFFFF, 0, 0, 0, width, height)
    bih = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, handler, width * height * 3, 0, 0, 0, 0)
    strl_v = _list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", bih))
    strl_a = b""
    if audio:
        strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 7, 0, 0xFFFFFFFF, 1, 0, 0, 0, 0)
        wfx = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        strl_a = _list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", wfx))
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + strl_a + strl_v)
    chunks = [_chunk(tag, f) for f in frames]
    n_rec = 2 if rec and len(frames) >= 2 else 0
    movi = b""
    if n_rec:
        movi += _list(b"rec ", chunks[0] + (_chunk(b"00wb", b"\x80" * 7) if audio else b"") + chunks[1])
    movi += _chunk(b"JUNK", b"\0" * 5)
    for c in chunks[n_rec:]:
        movi += c
        if audio:
            movi += _chunk(b"00wb", b"\x80" * 3)
    body = riff_kind + hdrl + _list(b"movi", movi)
    return b"RIFF" + struct.pack("<I", len(body)) + body
