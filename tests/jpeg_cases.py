"""A NumPy restatement of the whole JPEG decoder (baseline, one interleaved scan; include/lwpose.h's JPEG section) and the
fixtures of tests/golden/jpeg_*.npz.  The restatement is the oracle of test_jpeg_host.py / test_gpu_jpeg.py; it is itself pinned
against Pillow's pixels (libjpeg-turbo), which tools/make_jpeg_golden.py stored next to each file.  It decodes valid files only:
refusals are the library's business.

Mutation knobs (``row_first``, ``swap_7_8``) build deliberately wrong decoders: the tests use them to show that they would see
a transposed pass order or swapped h2v2 rounding constants."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


def _huff_lookup(counts, vals):
    """16-bit prefix -> (length, symbol) arrays of one canonical Huffman table (length 0: no code)."""
    length = np.zeros(1 << 16, dtype=np.uint8)
    symbol = np.zeros(1 << 16, dtype=np.uint8)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            first = code << (16 - l)
            length[first:first + (1 << (16 - l))] = l
            symbol[first:first + (1 << (16 - l))] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), symbol.tolist()


def parse(data):
    """The header fields, tables and the position of the entropy-coded data of a baseline file."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    pos = 2
    qt = np.zeros((4, 64), dtype=np.uint16)
    huff = {}
    hd = {"restart_interval": 0, "orientation": 0}
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        L = int.from_bytes(data[pos:pos + 2], "big")
        seg = data[pos + 2:pos + L]
        pos += L
        if m == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                qt[seg[0] & 15, ZIGZAG] = np.frombuffer(seg[1:65], dtype=np.uint8)
                seg = seg[65:]
        elif m == 0xC4:
            while seg:
                counts = list(seg[1:17])
                n = sum(counts)
                huff[(seg[0] >> 4, seg[0] & 15)] = _huff_lookup(counts, list(seg[17:17 + n]))
                seg = seg[17 + n:]
        elif m == 0xC0:
            assert seg[0] == 8
            hd["height"], hd["width"] = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            nf = seg[5]
            hd["components"] = nf
            hd["h_samp"] = [seg[7 + 3 * c] >> 4 for c in range(nf)]
            hd["v_samp"] = [seg[7 + 3 * c] & 15 for c in range(nf)]
            hd["quant_table"] = [seg[8 + 3 * c] for c in range(nf)]
            if nf == 1:
                hd["h_samp"], hd["v_samp"] = [1], [1]
        elif m == 0xDD:
            hd["restart_interval"] = int.from_bytes(seg[:2], "big")
        elif m == 0xE1 and seg[:6] == b"Exif\0\0":
            t = seg[6:]
            bo = "little" if t[:2] == b"II" else "big"
            ifd = int.from_bytes(t[4:8], bo)
            for i in range(int.from_bytes(t[ifd:ifd + 2], bo)):
                e = t[ifd + 2 + 12 * i:ifd + 14 + 12 * i]
                if int.from_bytes(e[:2], bo) == 0x0112:
                    hd["orientation"] = int.from_bytes(e[8:10], bo)
        elif m == 0xDA:
            ns = seg[0]
            hd["td"] = [seg[2 + 2 * c] >> 4 for c in range(ns)]
            hd["ta"] = [seg[2 + 2 * c] & 15 for c in range(ns)]
            break
    hmax, vmax = max(hd["h_samp"]), max(hd["v_samp"])
    hd["mcus_x"] = -(-hd["width"] // (8 * hmax))
    hd["mcus_y"] = -(-hd["height"] // (8 * vmax))
    hd["blocks_w"] = [hd["mcus_x"] * h for h in hd["h_samp"]]
    hd["blocks_h"] = [hd["mcus_y"] * v for v in hd["v_samp"]]
    hd["total_blocks"] = sum(w * h for w, h in zip(hd["blocks_w"], hd["blocks_h"]))
    return hd, qt, huff, pos


def decode_blocks(data):
    """(header, coefficients, qtables): the coefficients as the library lays them out, int16 (total_blocks, 64) in natural order
    and plane order, DC prediction undone, not dequantised."""
    data = bytes(data)
    hd, qt, huff, pos = parse(data)
    # the scan's intervals, un-stuffed; a marker ends each
    intervals, cur = [], bytearray()
    while True:
        b = data[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
        elif data[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
        elif data[pos + 1] == 0xFF:
            pos += 1
        else:
            intervals.append(bytes(cur))
            cur = bytearray()
            if not 0xD0 <= data[pos + 1] <= 0xD7:
                break
            pos += 2
    nc = hd["components"]
    planes = [np.zeros((hd["blocks_h"][c], hd["blocks_w"][c], 64), dtype=np.int16) for c in range(nc)]
    zz = ZIGZAG.tolist()
    n_mcus = hd["mcus_x"] * hd["mcus_y"]
    per = hd["restart_interval"] or n_mcus
    mcu = 0
    for chunk in intervals:
        buf = chunk + b"\0\0\0\0"
        bit = 0
        pred = [0] * nc

        def peek16():
            p = bit >> 3
            return (int.from_bytes(buf[p:p + 3], "big") >> (8 - (bit & 7))) & 0xFFFF

        for _ in range(min(per, n_mcus - mcu)):
            my, mx = divmod(mcu, hd["mcus_x"])
            for c in range(nc):
                dl, ds = huff[(0, hd["td"][c])]
                al, as_ = huff[(1, hd["ta"][c])]
                for v in range(hd["v_samp"][c]):
                    for u in range(hd["h_samp"][c]):
                        blk = [0] * 64
                        w = peek16()
                        assert dl[w]
                        bit += dl[w]
                        s = ds[w]
                        if s:
                            val = peek16() >> (16 - s)
                            bit += s
                            pred[c] += val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            w = peek16()
                            assert al[w]
                            bit += al[w]
                            rs = as_[w]
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            val = peek16() >> (16 - s)
                            bit += s
                            blk[zz[k]] = val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                            k += 1
                        planes[c][my * hd["v_samp"][c] + v, mx * hd["h_samp"][c] + u] = blk
            mcu += 1
        assert bit <= 8 * len(chunk)
    assert mcu == n_mcus
    coef = np.concatenate([p.reshape(-1, 64) for p in planes])
    return hd, coef, qt


def _idct8(x, axis, shift):
    """jidctint.c's 8-point pass along ``axis`` of an int64 array, descaled by ``shift`` with round-half-up."""
    i = [np.take(x, k, axis=axis) for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    e2 = z1 + i[6] * -15137
    e3 = z1 + i[2] * 6270
    e0, e1 = (i[0] + i[4]) * 8192, (i[0] - i[4]) * 8192
    t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (shift - 1)
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([(o + half) >> shift for o in out], axis=axis)


def idct_planes(hd, coef, qt, row_first=False):
    """The block-padded uint8 component planes, and the (min, max) of the IDCT output before the + 128."""
    planes, lo, hi, b0 = [], 0, 0, 0
    for c in range(hd["components"]):
        bw, bh = hd["blocks_w"][c], hd["blocks_h"][c]
        blk = coef[b0:b0 + bw * bh].astype(np.int64) * qt[hd["quant_table"][c]].astype(np.int64)
        b0 += bw * bh
        blk = blk.reshape(-1, 8, 8)                     # [block][row][column]
        if row_first:
            blk = _idct8(_idct8(blk, 2, 11), 1, 18)
        else:
            blk = _idct8(_idct8(blk, 1, 11), 2, 18)     # each column first, then each row
        lo, hi = min(lo, int(blk.min())), max(hi, int(blk.max()))
        px = np.clip(blk + 128, 0, 255).astype(np.uint8)
        planes.append(px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return planes, (lo, hi)


def _upsample(c, mode, swap_7_8=False):
    """Fancy up-sampling of one chroma plane at its TRUE size to int32 (2w wide; 2h high for h2v2)."""
    c = c.astype(np.int32)
    if mode == 1:
        return c
    left = np.concatenate([c[:, :1], c[:, :-1]], axis=1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    if mode == 2:
        out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int32)
        out[:, 0::2] = (3 * c + left + 1) >> 2
        out[:, 1::2] = (3 * c + right + 2) >> 2
        return out
    up = np.concatenate([c[:1], c[:-1]], axis=0)
    down = np.concatenate([c[1:], c[-1:]], axis=0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), dtype=np.int32)
    a, b = (7, 8) if swap_7_8 else (8, 7)
    for parity, far in ((0, up), (1, down)):
        s = 3 * c + far
        sl = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        sr = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[parity::2, 0::2] = (3 * s + sl + a) >> 4
        out[parity::2, 1::2] = (3 * s + sr + b) >> 4
    return out


def planes_to_bgr(hd, planes, swap_7_8=False):
    H, W = hd["height"], hd["width"]
    y = planes[0][:H, :W].astype(np.int32)
    if hd["components"] == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    hs, vs = hd["h_samp"][0], hd["v_samp"][0]
    mode = 1 if hs == 1 else 2 if vs == 1 else 3
    cw, ch = -(-W // hs), -(-H // vs)
    cb = _upsample(planes[1][:ch, :cw], mode, swap_7_8)[:H, :W] - 128
    cr = _upsample(planes[2][:ch, :cw], mode, swap_7_8)[:H, :W] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def decode_bgr(data, row_first=False, swap_7_8=False, want_range=False):
    hd, coef, qt = decode_blocks(data)
    planes, rng = idct_planes(hd, coef, qt, row_first)
    img = planes_to_bgr(hd, planes, swap_7_8)
    return (img, rng) if want_range else img


_FIXTURES = None


def fixtures():
    """{name: (jpeg bytes, Pillow's pixels as BGR uint8 (H, W, 3))} of every tests/golden/jpeg_*.npz, loaded once."""
    global _FIXTURES
    if _FIXTURES is None:
        out = {}
        for path in sorted(glob.glob(os.path.join(GOLDEN, "jpeg_*.npz"))):
            with np.load(path) as z:
                for name in [k[5:] for k in z.files if k.startswith("jpeg/")]:
                    rgb = z["rgb/" + name]
                    if rgb.ndim == 2:
                        rgb = np.repeat(rgb[:, :, None], 3, axis=2)
                    out[name] = (z["jpeg/" + name].tobytes(), np.ascontiguousarray(rgb[:, :, ::-1]))
        _FIXTURES = out
    return _FIXTURES


_RESTATED = {}


def restated(name):
    """(header, coefficients, qtables) of a fixture by the restatement, computed once per process."""
    if name not in _RESTATED:
        _RESTATED[name] = decode_blocks(fixtures()[name][0])
    return _RESTATED[name]
