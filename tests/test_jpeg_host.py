"""CPU: the JPEG reader without a GPU.  The NumPy restatement (jpeg_cases) against Pillow's pixels in the fixtures, which pins
the oracle; the host half of the library (marker parse, Huffman decode) against the restatement; every refusal the header
lists; prefixes and single-byte changes that must never crash; and the same walk in a stand-alone program under the host
compiler's address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine

import jpeg_cases as jc

from conftest import GOLDEN, ROOT

NEW_EXPORTS = ["lwp_jpeg_info", "lwp_debug_jpeg_blocks", "lwp_jpeg_decode_batch", "lwp_time_jpeg_decode_batch"]
FIX = jc.fixtures()
SMALL = "17x17_420"                                  # partial MCUs both ways, three tables of each kind


def refused(data):
    """The message of the ValueError both host entry points raise for ``data`` (they must agree that it is refused)."""
    with pytest.raises(ValueError) as e:
        Engine.debug_jpeg_blocks(data)
    return str(e.value)


def segment_at(data, marker):
    """Offset of the first 0xFF ``marker`` of the headers."""
    return data.index(bytes([0xFF, marker]))


def test_new_exports_are_declared_and_present():
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "lwpose.h")) as f:
        declared = set(re.findall(r"\b(lwp_[a-z_0-9]+)\s*\(", f.read()))
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name in declared, name
    assert L.lwp_version() >= 106


def test_the_fixtures_cover_the_listed_shapes():
    for w, h in [(1, 1), (8, 8), (16, 16), (17, 17), (9, 31), (33, 16), (16, 33), (37, 53)]:
        for s in ("444", "422", "420"):
            data, bgr = FIX["%dx%d_%s" % (w, h, s)]
            assert bgr.shape == (h, w, 3)
            hd = Engine.jpeg_info(data)
            assert (hd["h_samp"][0], hd["v_samp"][0]) == {"444": (1, 1), "422": (2, 1), "420": (2, 2)}[s]
    assert Engine.jpeg_info(FIX["grey_19x21"][0])["components"] == 1
    assert Engine.jpeg_info(FIX["restart2_37x53_420"][0])["restart_interval"] == 2
    assert b"\xff\xff\xd0" in FIX["fill_bytes_33x16_422"][0]


@pytest.mark.parametrize("name", sorted(FIX))
def test_restatement_equals_pillow_in_every_byte(name):
    data, bgr = FIX[name]
    img, (lo, hi) = jc.decode_bgr(data, want_range=True)
    assert img.shape == bgr.shape and int((img != bgr).sum()) == 0
    assert -512 <= lo and hi <= 511                  # beyond, libjpeg's range-limit table wraps where the project clamps


def test_restatement_equals_pillow_on_a_real_file():
    with np.load(os.path.join(GOLDEN, "jpeg_extra.npz")) as z:
        data, window, (oy, ox), shape, crc = z["jpeg"].tobytes(), z["window"], z["origin"], tuple(z["shape"]), int(z["crc32"][0])
    rgb = jc.decode_bgr(data)[:, :, ::-1]
    assert rgb.shape == shape
    assert np.array_equal(rgb[oy:oy + 256, ox:ox + 256], window)
    assert zlib.crc32(np.ascontiguousarray(rgb).tobytes()) == crc
    hd, coef, qt = Engine.debug_jpeg_blocks(data)
    _, coef_ref, qt_ref = jc.decode_blocks(data)
    assert np.array_equal(coef, coef_ref) and np.array_equal(qt, qt_ref)


def test_mutated_restatements_differ_from_the_fixtures():
    """The tests can see a transposed pass order and swapped h2v2 rounding constants."""
    assert any((jc.decode_bgr(d, row_first=True) != bgr).any() for d, bgr in FIX.values())
    names_420 = [n for n in FIX if n.endswith("_420")]
    assert any((jc.decode_bgr(FIX[n][0], swap_7_8=True) != FIX[n][1]).any() for n in names_420)


@pytest.mark.parametrize("name", sorted(FIX))
def test_host_blocks_equal_the_restatement(name):
    data = FIX[name][0]
    hd_ref, coef_ref, qt_ref = jc.restated(name)
    hd, coef, qt = Engine.debug_jpeg_blocks(data)
    assert coef.shape == coef_ref.shape and np.array_equal(coef, coef_ref)
    assert np.array_equal(qt, qt_ref)
    for key in ("width", "height", "components", "h_samp", "v_samp", "quant_table", "restart_interval", "mcus_x", "mcus_y",
                "orientation", "blocks_w", "blocks_h", "total_blocks"):
        assert hd[key] == hd_ref[key], key


def test_info_fields():
    hd = Engine.jpeg_info(FIX["37x53_420"][0])
    assert hd == {"width": 37, "height": 53, "components": 3, "h_samp": [2, 1, 1], "v_samp": [2, 1, 1], "quant_table": [0, 1, 1],
                  "restart_interval": 0, "mcus_x": 3, "mcus_y": 4, "orientation": 0, "blocks_w": [6, 3, 3], "blocks_h": [8, 4, 4],
                  "total_blocks": 72}
    assert Engine.jpeg_info(FIX["exif6_16x16_420"][0])["orientation"] == 6
    g = Engine.jpeg_info(FIX["grey_2x2_19x21"][0])       # one component: one block per MCU whatever the header states
    assert (g["h_samp"], g["v_samp"], g["blocks_w"], g["blocks_h"]) == ([1], [1], [3], [3])
    hd = _lib.JpegHeader()
    assert _lib.lib().lwp_jpeg_info(None, 0, C.byref(hd)) == _lib.LWP_ERR_ARG


def test_capacity_of_the_coefficient_buffer():
    data = FIX[SMALL][0]
    n = Engine.jpeg_info(data)["total_blocks"] * 64
    coef, qt = np.zeros(n, dtype=np.int16), np.zeros(256, dtype=np.uint16)
    L = _lib.lib()
    assert L.lwp_debug_jpeg_blocks(data, len(data), coef.ctypes.data, n - 1, qt.ctypes.data) == _lib.LWP_ERR_CAPACITY
    assert L.lwp_debug_jpeg_blocks(data, len(data), coef.ctypes.data, n, qt.ctypes.data) == _lib.LWP_OK


def patched(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


def test_every_listed_refusal_is_refused_with_its_reason():
    data = FIX[SMALL][0]
    sof = segment_at(data, 0xC0)
    for marker, word in ((0xC1, "SOF1"), (0xC2, "progressive"), (0xC3, "SOF3"), (0xC9, "arithmetic"), (0xCA, "arithmetic")):
        msg = refused(patched(data, sof + 1, [marker]))
        assert word in msg and "byte %d" % sof in msg, msg
    assert "12-bit" in refused(patched(data, sof + 4, [12]))
    assert "height of 0" in refused(patched(data, sof + 5, [0, 0]))
    assert "width of 0" in refused(patched(data, sof + 7, [0, 0]))
    assert "4 components" in refused(patched(data, sof + 9, [4]))
    for hv in (0x12, 0x41, 0x31, 0x14):                # 4:4:0, 4:1:1, 3x1, 1x4
        assert "sampling" in refused(patched(data, sof + 11, [hv])), hex(hv)
    assert "sampling" in refused(patched(data, sof + 14, [0x21]))          # chroma not 1x1
    # Adobe APP14: transform 1 passes, 0 and 2 are refused
    def adobe(t):
        return data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([t]) + data[2:]
    hd, coef, _ = Engine.debug_jpeg_blocks(adobe(1))
    assert np.array_equal(coef, jc.restated(SMALL)[1])
    for t in (0, 2):
        assert "Adobe colour transform %d" % t in refused(adobe(t))
    # several scans: a scan header that lists one of the three components
    sos = segment_at(data, 0xDA)
    one = data[:sos] + b"\xff\xda\x00\x08\x01" + data[sos + 5:sos + 7] + data[sos + 11:]
    assert "several scans" in refused(one)
    # a second scan behind the first
    eoi = len(data) - 2
    assert data[eoi:] == b"\xff\xd9"
    assert "second scan" in refused(data[:eoi] + data[sos:])
    assert "DNL" in refused(data[:eoi] + b"\xff\xdc\x00\x04\x00\x35\xff\xd9")
    assert "DNL" in refused(data[:sos] + b"\xff\xdc\x00\x04\x00\x35" + data[sos:])
    assert "arithmetic" in refused(data[:sos] + b"\xff\xcc\x00\x04\x00\x10" + data[sos:])
    dqt = segment_at(data, 0xDB)
    assert "Pq = 1" in refused(patched(data, dqt + 4, [0x10]))
    # missing tables: the scan names one nobody defined
    assert "Huffman table 3" in refused(patched(data, sos + 6, [0x30]))
    assert "Huffman table 2" in refused(patched(data, sos + 6, [0x02]))
    assert "quantisation table 3" in refused(patched(data, sof + 12, [3]))
    # malformed streams
    assert "runs past the end" in refused(patched(data, dqt + 2, [0xFF, 0xFF]))
    assert "ends before the last MCU" in refused(data[:eoi - 6] + b"\xff\xd9")
    assert "truncated" in refused(data[:sos + 3])
    assert "EOI" in refused(data[:eoi])
    assert "not a JPEG" in refused(b"\x89PNG" + data[4:])
    r = FIX["restart2_33x16_422"][0]
    rst = r.index(b"\xff\xd1")
    assert "RST1 is missing or wrong" in refused(patched(r, rst + 1, [0xD2]))
    assert "RST1 is missing or wrong" in refused(r[:rst] + r[rst + 2:])
    assert "DRI" in refused(patched(r, segment_at(r, 0xDD) + 3, [5]))


def dht_file(dc_counts, dc_vals, ac_counts, ac_vals, scan, w=8, h=8):
    """A grey w x h file around hand-made Huffman tables and scan bytes."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = b"\xff\xd8" + seg(0xDB, [0] + [1] * 64)
    out += seg(0xC0, [8] + list(h.to_bytes(2, "big")) + list(w.to_bytes(2, "big")) + [1, 1, 0x11, 0])
    out += seg(0xC4, [0x00] + dc_counts + dc_vals) + seg(0xC4, [0x10] + ac_counts + ac_vals)
    out += seg(0xDA, [1, 1, 0x00, 0, 63, 0])
    return out + bytes(scan) + b"\xff\xd9"


def counts(**at):
    c = [0] * 16
    for k, v in at.items():
        c[int(k[1:]) - 1] = v
    return c


def test_entropy_errors_are_refused():
    # a valid hand-made block first: DC category 2 (code 0), value bits 11 -> 3; AC (0, 1) (code 0) + bit 1, then EOB (code 10)
    dc, ac = (counts(l1=1), [2]), (counts(l1=1, l2=1), [0x01, 0x00])
    hd, coef, qt = Engine.debug_jpeg_blocks(dht_file(*dc, *ac, scan=[0b01101101]))
    assert coef[0, 0] == 3 and coef[0, 1] == 1 and not coef[0, 2:].any() and (qt[0] == 1).all()
    # DC category 12
    assert "DC category of 12" in refused(dht_file(counts(l1=1), [12], *ac, scan=[0b01111111, 0x7F]))
    # AC size 11
    assert "AC size of 11" in refused(dht_file(*dc, counts(l1=1), [0x0B], scan=[0b01101111, 0x7F]))
    # a code that matches no symbol: one DC code '0' only, the scan starts with sixteen ones
    assert "matches no symbol" in refused(dht_file(*dc, *ac, scan=[0xFF, 0x00, 0xFF, 0x00, 0xFF, 0x00]))
    # a run past coefficient 63: AC symbol (15, 1) five times
    run = dht_file(*dc, counts(l1=1), [0xF1], scan=[0b01100000, 0b00000000, 0])
    assert "past 63" in refused(run)
    # ZRL four times
    assert "past 63" in refused(dht_file(*dc, counts(l1=1), [0xF0], scan=[0b01100000, 0]))
    # code lengths that describe no prefix code: three codes of length 1
    assert "no prefix code" in refused(dht_file(counts(l1=3), [0, 1, 2], *ac, scan=[0]))
    # a DC value outside 8-bit data's range: category 11 diffs of +2047 and +1024 (a 16 x 8 file has two blocks)
    big = dht_file(counts(l1=1), [11], counts(l1=1), [0x00], scan=[0x7F, 0xF2, 0x00, 0x3F], w=16)
    assert "DC value" in refused(big)


def test_prefixes_and_single_byte_changes_never_crash():
    L = _lib.lib()
    hd = _lib.JpegHeader()
    coef, qt = np.zeros(64 * 4096, dtype=np.int16), np.zeros(256, dtype=np.uint16)
    allowed = (_lib.LWP_OK, _lib.LWP_ERR_ARG, _lib.LWP_ERR_CAPACITY)
    for name in (SMALL, "restart2_33x16_422"):
        data = FIX[name][0]
        for n in range(len(data)):
            assert L.lwp_jpeg_info(data[:n], n, C.byref(hd)) in allowed
            assert L.lwp_debug_jpeg_blocks(data[:n], n, coef.ctypes.data, coef.size, qt.ctypes.data) == _lib.LWP_ERR_ARG, n
    data = FIX["1x1_444"][0]
    buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
    n_ok = 0
    for i in range(len(data)):
        for v in range(1, 256):
            buf[i] = data[i] ^ v
            rc = L.lwp_debug_jpeg_blocks(buf, len(data), coef.ctypes.data, coef.size, qt.ctypes.data)
            assert rc in allowed, (i, v, rc)
            n_ok += rc == _lib.LWP_OK
        buf[i] = data[i]
    assert 0 < n_ok < 255 * len(data)                # some changes are harmless (a quantiser, a comment), most are refused


def host_compiler_with_sanitizers(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    for cxx in ("g++", "clang++", "c++"):
        exe = shutil.which(cxx)
        if exe is None:
            continue
        r = subprocess.run([exe, "-fsanitize=address,undefined", str(src), "-o", str(tmp_path / "probe")], capture_output=True)
        if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0:
            return exe
    return None


def test_stand_alone_walk_under_the_sanitizers(tmp_path):
    cxx = host_compiler_with_sanitizers(tmp_path)
    if cxx is None:
        pytest.skip("no host compiler accepts -fsanitize=address,undefined")
    pkg = os.path.join(ROOT, "lightweight-human-pose-estimation.pytorch_amd", "csrc")
    exe = str(tmp_path / "jpeg_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(pkg, "jpeg_host.cpp"), os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", exe], check=True)
    files = []
    for name in (SMALL, "restart2_33x16_422", "grey_19x21", "optimised_37x53_420", "1x1_444", "8x8_422"):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(FIX[name][0])
        files.append(str(path))
    r = subprocess.run([exe] + files[:4] + ["--mutate"] + files[4:], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused" in r.stdout
