"""CPU: the JPEG encoder's fixed points without a GPU.  The NumPy restatement of the forward path
(tests/jpeg_encode_cases.py) against the coefficients in the files Pillow wrote; restatement + jpeg_entropy_cases' scan coder + the
library's header bytes against every byte of those files; the quality tables; mutants of the restatement, to show that the
fixtures bite; the Motion-JPEG containers with a stub engine; the argument checks."""
import io
import struct

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.datasets import coco
from lwpose_amd.runtime import Engine

import jpeg_cases as jc
import jpeg_encode_cases as jen

from conftest import GOLDEN

FIX = jen.fixtures()
NAMES = sorted(FIX)
# what the long fixture must span (csrc/lwp_internal.h): kJpegEncGroup blocks a workgroup of the length and write passes and a
# tile of the offset scan; kJpegEncGroup * kJpegEncChunk un-stuffed bytes a tile of the stuffing passes
ENC_GROUP, ENC_CHUNK = 256, 32


def test_the_fixtures_cover_what_the_issue_lists():
    assert len(NAMES) >= 50
    sizes = {FIX[n]["bgr"].shape[:2] for n in NAMES}
    assert {(1, 1), (7, 7), (8, 9), (16, 32), (17, 23), (24, 17), (24, 25), (40, 9), (33, 50), (31, 65), (100, 75)} <= sizes
    for hw in sizes - {(75, 100)}:
        assert {FIX[n]["sampling"] for n in NAMES if FIX[n]["bgr"].shape[:2] == hw} == set(jen.SAMPLINGS), hw
    assert {FIX[n]["quality"] for n in NAMES} >= {1, 30, 75, 95, 100}
    for s in ("444", "422", "420"):
        g = jen.geometry(50, 33, {v: k for k, v in jen.SHORT.items()}[s])
        assert FIX["restart1_50x33_" + s]["restart"] == 1 and FIX["restartrow_50x33_" + s]["restart"] == g["mcus_x"]
        assert FIX["restartbig_23x17_" + s]["restart"] > jen.geometry(23, 17, "4:4:4")["mcus_x"] * 3
        assert jen.geometry(65, 31, "4:4:4")["mcus_x"] > 8           # restart1_many: the RSTn numbering wraps
        assert not FIX["zeros_17x24_" + s]["bgr"].any() and FIX["ones_25x24_" + s]["bgr"].min() == 255
        assert set(np.unique(FIX["checker_23x17_" + s]["bgr"])) == {0, 255}
    f = FIX["long_100x75_444_q100"]
    g, _, _ = jen.restated("long_100x75_444_q100")
    scan = f["jpeg"][f["jpeg"].index(b"\xff\xda") + 14:-2]
    assert g["total_blocks"] > ENC_GROUP and len(scan.replace(b"\xff\x00", b"\xff")) > ENC_GROUP * ENC_CHUNK
    assert scan.count(b"\xff\x00") > 50                           # noise at quality 100: many stuffed bytes
    assert sum(len(FIX[n]["jpeg"]) + FIX[n]["bgr"].size for n in NAMES) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_gives_the_coefficients_in_pillows_file(name):
    f = FIX[name]
    hd, want, qt = jc.decode_blocks(f["jpeg"])
    g, got, qt_got = jen.restated(name)
    assert hd["restart_interval"] == f["restart"] and hd["h_samp"][0] == g["h_samp"][0] and hd["v_samp"][0] == g["v_samp"][0]
    assert got.shape == want.shape and got.dtype == np.int16
    assert int((got != want).sum()) == 0, "%d of %d coefficients differ" % (int((got != want).sum()), want.size)
    assert np.array_equal(qt, qt_got)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_scan_coder_and_the_librarys_header_give_pillows_file_in_every_byte(name):
    f = FIX[name]
    H, W = f["bgr"].shape[:2]
    header = Engine.debug_jpeg_encode_header(H, W, f["quality"], f["sampling"], f["restart"])
    g, coef, _ = jen.restated(name)
    data = header + jen.scan_of(coef, g, f["restart"]) + b"\xff\xd9"
    assert data[:len(header)] == f["jpeg"][:len(header)], "the header differs"
    assert data == f["jpeg"]
    assert len(header) == (629 if f["restart"] else 623) <= 640
    assert len(f["jpeg"]) <= Engine.jpeg_encode_bound(H, W, f["sampling"], f["restart"])
    info = Engine.jpeg_info(header)                                 # the reader's parse of the writer's header
    assert (info["height"], info["width"], info["components"], info["restart_interval"]) == (H, W, 3, f["restart"])
    assert info["total_blocks"] == g["total_blocks"] and info["blocks_w"] == g["blocks_w"] and info["blocks_h"] == g["blocks_h"]


def test_the_quality_tables_of_1_to_100_are_pillows():
    with np.load(GOLDEN + "/encjpeg_tables.npz") as z:
        tables = z["tables"]
    assert tables.shape == (100, 2, 64)
    assert (tables[0] == 255).all()                                 # quality 1: every entry clamps at 255
    assert tables[99].max() == 1                                    # quality 100: all ones
    for q in range(1, 101):
        assert np.array_equal(jen.quality_tables(q)[:2], tables[q - 1]), q
        _, qt, _, _ = jc.parse(Engine.debug_jpeg_encode_header(8, 8, q, "4:4:4") + b"\xff\xd9")
        assert np.array_equal(qt[:2], tables[q - 1]) and not qt[2:].any(), q


@pytest.mark.parametrize("mutant,name", [
    ("bottom_before_downsample", "noise_9x8_420_q95"), ("bottom_before_downsample", "noise_17x24_420_q75"),
    ("bottom_before_downsample", "noise_9x40_420_q95"),
    ("replicate_right", "noise_23x17_422_q95"), ("replicate_right", "noise_17x24_420_q75"), ("replicate_right", "noise_50x33_420_q30"),
    ("constant_bias", "noise_9x8_422_q75"), ("constant_bias", "noise_9x8_420_q95"),
    ("truncating_quantiser", "noise_32x16_444_q100"), ("truncating_quantiser", "smooth_65x31_420")])
def test_a_mutant_of_the_restatement_fails_on_its_fixture(mutant, name):
    f = FIX[name]
    _, want, _ = jc.decode_blocks(f["jpeg"])
    _, got, _ = jen.forward_blocks(f["bgr"], f["sampling"], f["quality"], mutant)
    assert got.shape == want.shape and int((got != want).sum()) > 0


def test_the_bottom_rule_shows_only_where_the_padding_rows_exist():
    """H = 16 at 4:2:0 has no chroma padding rows (8 down-sampled rows fill the block): the mutant is invisible there, so the
    fixtures of H = 8, 24 and 40 are the ones that hold the rule."""
    f = FIX["noise_32x16_420_q30"]
    _, want, _ = jen.restated("noise_32x16_420_q30")
    _, got, _ = jen.forward_blocks(f["bgr"], f["sampling"], f["quality"], "bottom_before_downsample")
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- containers
class StubEngine(object):
    """Stands in for runtime.Engine: 'encodes' a frame as a tiny valid-looking JPEG that carries its bytes, 'decodes' a file
    to itself.  No GPU."""

    def __init__(self):
        self.decoded = []

    @staticmethod
    def _jpeg_encode_options(quality, subsampling, restart_interval):
        return Engine._jpeg_encode_options(quality, subsampling, restart_interval)

    def encode_jpeg_batch(self, frames, quality=75, subsampling="4:2:0", restart_interval=0):
        out = []
        for f in frames:
            body = bytes(np.asarray(f).reshape(-1)[:7 + int(np.asarray(f).reshape(-1)[0]) % 5].tolist()).replace(b"\xff", b"\xfe")
            out.append(b"\xff\xd8\xff\xc4\x00\x03\x00\xff\xda\x00\x02" + body + b"\xff\xd9")
        return out

    def decode_jpeg_batch(self, files, entropy=None):
        self.decoded.append(len(files))
        return list(files)


def frames_for_stub(n, h=4, w=6):
    return [np.full((h, w, 3), 3 * k + 1, dtype=np.uint8) for k in range(n)]


@pytest.mark.parametrize("container", ["avi", "mjpeg"])
def test_writer_to_bytes_to_reader_round_trips_the_payloads(container):
    eng = StubEngine()
    frames = frames_for_stub(7)
    want = eng.encode_jpeg_batch(frames)
    assert any(len(w) & 1 for w in want) and any(not len(w) & 1 for w in want)      # odd and even chunk lengths
    buf = io.BytesIO()
    with demo.VideoWriter(buf, eng, fps=25, container=container) as vw:
        vw.write(frames[0])
        vw.write(np.stack(frames[1:4]))
        vw.write(frames[4:])
    assert vw.frames == 7 and vw.size == (4, 6)
    data = buf.getvalue()
    reader = demo.VideoReader(data, eng, batch=3)
    assert list(reader) == want and eng.decoded == [3, 3, 1]
    assert list(reader) == want                                       # a second iteration starts over
    if container == "mjpeg":
        assert data == b"".join(want)
        return
    assert reader.fps == 25
    # the header fields close() patched, read by their place in the specification
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    assert data[12:16] == b"LIST" and data[20:24] == b"hdrl" and data[24:28] == b"avih" and struct.unpack_from("<I", data, 28)[0] == 56
    us, _, _, flags, total, _, streams, suggested, width, height = struct.unpack_from("<10I", data, 32)
    assert (us, flags & 0x10, total, streams, suggested, width, height) == (40000, 0x10, 7, 1, max(map(len, want)), 6, 4)
    strh = data.index(b"strh") + 8
    assert data[strh:strh + 8] == b"vidsMJPG" and struct.unpack_from("<I", data, strh + 32)[0] == 7
    assert struct.unpack_from("<II", data, strh + 20) == (1, 25)
    strf = data.index(b"strf") + 8
    assert struct.unpack_from("<I", data, strf - 4)[0] == 40 and struct.unpack_from("<Iii", data, strf) == (40, 6, 4)
    assert data[strf + 16:strf + 20] == b"MJPG"
    movi = data.index(b"movi")
    idx = data.index(b"idx1")
    assert data[movi - 8:movi - 4] == b"LIST" and movi + struct.unpack_from("<I", data, movi - 4)[0] == idx
    assert struct.unpack_from("<I", data, idx + 4)[0] == 16 * 7 and idx + 8 + 16 * 7 == len(data)
    for k, w in enumerate(want):
        ckid, fl, off, size = struct.unpack_from("<4sIII", data, idx + 8 + 16 * k)
        assert (ckid, fl, size) == (b"00dc", 0x10, len(w))
        assert data[movi + off:movi + off + 4] == b"00dc" and data[movi + off + 8:movi + off + 8 + size] == w
        assert (movi + off) % 2 == 0                                  # every chunk starts on an even offset


def test_the_reader_parses_hand_built_containers():
    eng = StubEngine()
    files = eng.encode_jpeg_batch(frames_for_stub(5))
    no_dht = jen.strip_dht(files[2])
    assert b"\xff\xc4" not in no_dht
    stored = [files[0], files[1], no_dht, b"", files[4]]                # frame 2 without DHT, frame 3 dropped
    avi = jen.build_avi(stored, 6, 4, fps=12)
    assert b"rec " in avi and b"auds" in avi and b"00wb" in avi and b"JUNK" in avi and b"01dc" in avi
    got = list(demo.VideoReader(avi, eng, batch=2))
    spliced = got[2]
    assert got == [files[0], files[1], spliced, spliced, files[4]]      # the dropped frame repeats the one before it
    assert spliced != no_dht and spliced.replace(jen.dht_segments(), b"") == no_dht
    assert spliced.index(jen.dht_segments()) + len(jen.dht_segments()) == spliced.index(b"\xff\xda")
    reader = demo.VideoReader(avi, eng)
    assert reader.fps is None and len(list(reader)) == 5 and reader.fps == 12      # the header is read when the iteration starts
    # the same frames as a bare stream of JPEG files (no dropped frame there: the container has no way to say so)
    mj = b"".join(s for s in stored if s)
    assert list(demo.VideoReader(mj, eng, batch=8)) == [files[0], files[1], spliced, files[4]]
    # a dropped first frame has nothing to repeat
    assert list(demo.VideoReader(jen.build_avi([b"", files[1]], 6, 4, audio=False, rec=False), eng)) == [files[1]]


def test_the_spliced_tables_make_a_real_frame_decodable_again():
    f = FIX["noise_23x17_420_q100"]
    bare = jen.strip_dht(f["jpeg"])
    assert len(bare) == len(f["jpeg"]) - len(jen.dht_segments())
    with pytest.raises(ValueError, match="Huffman table .* missing"):
        Engine.jpeg_info(bare)
    assert demo._prepare_frame(bare, 0) == f["jpeg"]                    # Pillow's own layout: the tables stand in front of SOS
    assert demo._prepare_frame(f["jpeg"], 0) == f["jpeg"]


def test_what_the_reader_refuses(tmp_path):
    eng = StubEngine()
    files = eng.encode_jpeg_batch(frames_for_stub(2))
    with pytest.raises(ValueError, match="camera index"):
        demo.VideoReader(0, eng)
    with pytest.raises(ValueError, match="camera index"):
        demo.VideoReader("1", eng)
    with pytest.raises(ValueError, match="batch"):
        demo.VideoReader(b"", eng, batch=0)
    with pytest.raises(OSError):
        iter(demo.VideoReader(str(tmp_path / "missing.avi"), eng))
    with pytest.raises(ValueError, match="H264.*MJPG"):
        iter(demo.VideoReader(jen.build_avi(files, 6, 4, handler=b"H264"), eng))
    with pytest.raises(ValueError, match="AVIX"):
        iter(demo.VideoReader(jen.build_avi(files, 6, 4, riff_kind=b"AVIX"), eng))
    opendml = jen.build_avi(files, 6, 4) + b"RIFF" + struct.pack("<I", 4) + b"AVIX"
    with pytest.raises(ValueError, match="OpenDML"):
        iter(demo.VideoReader(opendml, eng))
    field = files[0][:2] + b"\xff\xe0\x00\x10AVI1\x01" + b"\0" * 9 + files[0][2:]
    with pytest.raises(ValueError, match="frame 1: an interlaced AVI1"):
        list(demo.VideoReader(jen.build_avi([files[0], field], 6, 4, audio=False), eng))
    progressive_field = files[0][:2] + b"\xff\xe0\x00\x10AVI1\x00" + b"\0" * 9 + files[0][2:]        # polarity 0: a whole frame
    assert len(list(demo.VideoReader(jen.build_avi([progressive_field], 6, 4, audio=False), eng))) == 1
    with pytest.raises(ValueError, match="neither"):
        iter(demo.VideoReader(b"GIF89a" + b"\0" * 20, eng))
    with pytest.raises(ValueError, match="truncated"):
        iter(demo.VideoReader(jen.build_avi(files, 6, 4)[:-9], eng))
    with pytest.raises(ValueError, match="no EOI"):
        iter(demo.VideoReader(files[0] + files[1][:-2], eng))


def test_what_the_writer_refuses_and_the_size_limit(tmp_path):
    eng = StubEngine()
    with pytest.raises(ValueError, match="avi"):
        demo.VideoWriter(str(tmp_path / "out.mp4"), eng)
    with pytest.raises(ValueError, match="quality"):
        demo.VideoWriter(io.BytesIO(), eng, quality=0, container="avi")
    with pytest.raises(ValueError, match="fps"):
        demo.VideoWriter(io.BytesIO(), eng, fps=0, container="avi")
    frames = frames_for_stub(6)
    path = str(tmp_path / "out.avi")
    vw = demo.VideoWriter(path, eng)
    vw.write(frames[0])
    with pytest.raises(ValueError, match="one size"):
        vw.write(np.zeros((5, 6, 3), np.uint8))
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        vw.write(np.zeros((4, 6), np.uint8))
    vw.close()
    vw.close()
    with pytest.raises(ValueError, match="closed"):
        vw.write(frames[1])
    assert list(demo.VideoReader(path, eng)) == eng.encode_jpeg_batch(frames[:1])
    # a file that would pass the limit is closed properly, index and all, and says so
    want = eng.encode_jpeg_batch(frames)
    whole = io.BytesIO()
    with demo.VideoWriter(whole, eng, container="avi") as vw:
        vw.write(frames)
    limit = len(whole.getvalue()) - 20                                  # room for five frames and their index, not for six
    buf = io.BytesIO()
    vw = demo.VideoWriter(buf, eng, container="avi")
    assert vw.max_bytes == 2 ** 31 - 1
    vw.max_bytes = limit
    vw.write(frames[:3])
    with pytest.raises(OverflowError, match="5 frames"):
        vw.write(frames[3:])
    with pytest.raises(ValueError, match="closed"):
        vw.write(frames[5])
    data = buf.getvalue()
    assert len(data) <= limit and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    assert list(demo.VideoReader(data, eng)) == want[:5]
    empty = io.BytesIO()
    demo.VideoWriter(empty, eng, container="avi").close()
    assert list(demo.VideoReader(empty.getvalue(), eng)) == []


def test_argument_checks_raise_without_a_gpu(tmp_path):
    assert _lib.lib().lwp_version() >= 109
    for bad in (0, 101, 75.0, "75", True, None):
        with pytest.raises(ValueError, match="quality"):
            Engine._jpeg_encode_options(bad, "4:2:0", 0)
    for bad in ("420", 2, None, "4:1:1", "4:4:0"):
        with pytest.raises(ValueError, match="subsampling"):
            Engine._jpeg_encode_options(75, bad, 0)
    for bad in (-1, 65536, 1.5):
        with pytest.raises(ValueError, match="restart_interval"):
            Engine._jpeg_encode_options(75, "4:2:0", bad)
    assert Engine._jpeg_encode_options(np.int64(1), "4:4:4", 65535) == (1, 0, 65535)
    for h, w in ((0, 8), (8, 0), (65536, 8), (8, 65536), (-1, 8)):
        with pytest.raises(ValueError, match="1..65535"):
            Engine.jpeg_encode_bound(h, w)
        with pytest.raises(ValueError, match="1..65535"):
            Engine.debug_jpeg_encode_header(h, w)
    assert Engine.jpeg_encode_bound(65535, 65535, "4:4:4") > 65535 * 65535
    n = _lib.C.c_size_t()
    small = np.zeros(100, np.uint8)
    rc = _lib.lib().lwp_debug_jpeg_encode_header(8, 8, 75, 2, 0, small.ctypes.data, small.size, _lib.C.byref(n))
    assert rc == _lib.LWP_ERR_CAPACITY and not small.any()
    with pytest.raises(ValueError, match="JPEG files"):
        coco.imwrite(str(tmp_path / "x.png"), np.zeros((4, 4, 3), np.uint8), StubEngine())
    assert coco.imwrite(str(tmp_path / "x.jpg"), np.full((4, 4, 3), 9, np.uint8), StubEngine()) is True
    assert (tmp_path / "x.jpg").read_bytes() == StubEngine().encode_jpeg_batch([np.full((4, 4, 3), 9, np.uint8)])[0]
    with pytest.raises(ValueError, match="unknown overlay option"):
        demo._overlay_options({"device": True, "colour": (1, 2, 3)})
    assert demo._overlay_options({"device": True, "boxes": False}) == ({"boxes": False}, True)
    assert demo._overlay_options(True) == ({}, False)


# ---------------------------------------------------------------------------------------------- the entropy stages' cases
# Conditions on the INPUTS of test_gpu_jpeg_encode_edges.py, read with the meter (jpeg_encode_cases.coverage) from the
# coefficients and the reference coder alone.  A case that misses its condition fails here; nothing is skipped.
CASES = jen.coefficient_cases()
EDGES = sorted(n for n in NAMES if n.startswith(("tiles_", "seam_")))
BLOCK_BYTES = 208                                                   # kJpegEncBlockBytes (csrc/jpeg_encode_host.h)

_METERS = {}


def meter(name):
    if name not in _METERS:
        if name in CASES:
            c = CASES[name]
            _METERS[name] = jen.coverage(c["coef"], c["g"], c["restart"])
        else:
            g, coef, _ = jen.restated(name)
            _METERS[name] = jen.coverage(coef, g, FIX[name]["restart"])
    return _METERS[name]


def reached(names):
    """The union over these cases or fixtures: (DC categories, AC symbols) per table."""
    dc, ac = [set(), set()], [set(), set()]
    for n in names:
        for t in (0, 1):
            dc[t] |= meter(n)["dc"][t]
            ac[t] |= meter(n)["ac"][t]
    return dc, ac


def test_the_edge_fixtures_are_the_ones_the_tool_writes():
    assert EDGES == sorted(["tiles_99x37_%s" % s for s in ("444", "422", "420")] + ["seam_144x64_%s" % s for s in ("444", "422", "420")])
    for n in EDGES:
        f = FIX[n]
        assert (f["quality"], f["restart"]) == ((100, 0) if n.startswith("tiles") else (75, 1)), n
    for s in ("444", "422", "420"):                                # DC categories 10 and 11 from pixels, in both tables
        m = meter("tiles_99x37_" + s)
        assert {10, 11} <= m["dc"][0] and {10, 11} <= m["dc"][1], (s, m["dc"])
    m = meter("seam_144x64_422")                                    # the tile seam through the whole pixel path
    assert ENC_GROUP in m["starts"] and len(m["starts"]) == 72


def test_what_the_older_fixtures_leave_to_the_coefficient_cases():
    """The gap the coefficient cases close, measured: without the edge fixtures no DC category above 9 in either table, 107
    and 94 of the 162 AC symbols (EOB and ZRL among them), no restart interval that starts on a tile seam of the offset scan,
    and no scan that ends in 0xFF."""
    old = [n for n in NAMES if n not in EDGES]
    assert len(old) == 59
    dc, ac = reached(old)
    assert max(dc[0]) == 9 and max(dc[1]) == 9
    assert (len(ac[0]), len(ac[1])) == (107, 94)
    assert not any(s and s % ENC_GROUP == 0 for n in old for s in meter(n)["starts"])
    assert not any(meter(n)["ff_last"] for n in old)
    assert sum(len(meter(n)["ff_ends"]) for n in old) == 14
    assert sum(b % ENC_CHUNK == 0 for n in old for b in meter(n)["start_bytes"][1:]) == 3


def test_alphabet_emits_every_symbol_of_all_four_tables():
    for name in ("alphabet_420", "alphabet_444"):
        m = meter(name)
        for t in (0, 1):
            assert m["ac"][t] == jen.ALL_AC and len(m["ac"][t]) == 162, (name, t, sorted(jen.ALL_AC - m["ac"][t]))
            assert m["dc"][t] == jen.ALL_DC, (name, t)
        assert m["max_zrl"] == 3                                    # a gap of 48 or more zeros
        assert 200 <= CASES[name]["g"]["total_blocks"] <= 400
    assert CASES["alphabet_420"]["sampling"] == "4:2:0" and CASES["alphabet_444"]["sampling"] == "4:4:4"


WORST = sorted(n for n in CASES if n.startswith("worst_"))


def test_worst_drives_every_luma_block_to_the_bound():
    assert len(WORST) == 8 and {(CASES[n]["sampling"], CASES[n]["size"], CASES[n]["restart"]) for n in WORST} == {
        ("4:2:0", (16, 16), 0), ("4:2:0", (16, 16), 1), ("4:4:4", (8, 24), 0), ("4:4:4", (8, 24), 1)}
    assert jen.WORST_BLOCK_BITS == 9 + 11 + 63 * (16 + 10) == 1658 <= 8 * BLOCK_BYTES
    for name in WORST:
        c, m = CASES[name], meter(name)
        _, comp = jen.jec.stream_order(c["g"])
        luma = [b for b, cc in zip(m["block_bits"], comp) if cc == 0]
        assert luma and set(luma) == {jen.WORST_BLOCK_BITS}, name
        assert max(m["block_bits"]) == jen.WORST_BLOCK_BITS, name   # chroma's code of run 0, size 10 is shorter: no block takes more
        assert m["dc"][0] == {11} and m["dc"][1] == {11} and m["ac"][0] == {0x0A}, name
        coef = c["coef"]
        assert coef[:, 0].min() == -1024 and coef[:, 0].max() <= 1023 and np.abs(coef[:, 1:].astype(np.int64)).max() <= 1023
        assert np.abs(coef[:, 1:].astype(np.int64)).min() >= 512
        # the un-stuffed scan inside what the planner gives it, the stuffed scan inside the bound of the API
        H, W = c["size"]
        intervals = len(m["starts"])
        assert m["length"] <= c["g"]["total_blocks"] * BLOCK_BYTES + intervals, name
        assert m["length"] >= c["g"]["total_blocks"] * 176, name    # and near it: 1408 bits is what a chroma block takes here
        header = Engine.debug_jpeg_encode_header(H, W, 75, c["sampling"], c["restart"])
        scan = jen.coefficient_scan(name)
        assert len(header) + len(scan) + 2 <= Engine.jpeg_encode_bound(H, W, c["sampling"], c["restart"]), name
        assert len(scan) <= Engine.jpeg_encode_bound(H, W, c["sampling"], c["restart"]) - 640 - 2, name
    ones = meter("worst_ones_444_r1")
    assert len(ones["ff"]) > ones["length"] // 2                    # all-ones magnitudes: more than every second byte is stuffed


def test_tile_seam_starts_an_interval_on_the_first_lane_of_a_later_tile():
    for restart, blocks in ((1, 4), (8, 32), (64, 256)):
        c, m = CASES["tile_seam_422_r%d" % restart], meter("tile_seam_422_r%d" % restart)
        assert (c["sampling"], c["size"], c["g"]["total_blocks"]) == ("4:2:2", (64, 144), 288)
        assert m["starts"] == list(range(0, 288, blocks)) and ENC_GROUP in m["starts"]
        assert sum(m["block_bits"][ENC_GROUP - blocks:ENC_GROUP]) % 8          # pad bits in front of the seam: the alignment does something
    c, m = CASES["tile_seam_420_r128"], meter("tile_seam_420_r128")
    assert c["sampling"] == "4:2:0" and c["g"]["total_blocks"] > 768 and m["starts"] == [0, 768] and 768 == 3 * ENC_GROUP
    assert m["length"] > ENC_GROUP * ENC_CHUNK                      # and more than one tile of the stuffing passes


def test_ends_in_ff_aligned_start_and_empty_codes():
    c, m = CASES["ends_in_ff"], meter("ends_in_ff")
    assert (c["size"], c["sampling"], c["restart"]) == ((8, 8), "4:4:4", 0)
    assert m["ff_last"] and jen.coefficient_scan("ends_in_ff")[-2:] == b"\xff\x00"
    m = meter("ends_in_ff_r1")
    assert CASES["ends_in_ff_r1"]["restart"] == 1 and m["ff_last"] and m["ff_ends"] and len(m["starts"]) == 3
    scan = jen.coefficient_scan("ends_in_ff_r1")
    assert scan[-2:] == b"\xff\x00" and (b"\xff\x00\xff\xd0" in scan or b"\xff\x00\xff\xd1" in scan)
    m = meter("aligned_start_r1")
    assert any(b % ENC_CHUNK == 0 for b in m["start_bytes"][1:])
    for name in ("empty_codes_444", "empty_codes_420"):
        c, m = CASES[name], meter(name)
        assert not c["coef"].any() and c["g"]["total_blocks"] > 200
        _, comp = jen.jec.stream_order(c["g"])
        assert all(b == (6 if cc == 0 else 4) for b, cc in zip(m["block_bits"], comp))      # DC category 0 and EOB
        offsets = np.cumsum([0] + m["block_bits"][:-1])
        assert set(int(o) % 8 for o in offsets) == set(range(0, 8, 2)) and not m["ff"]      # every even bit offset; words shared by 5 blocks


def test_many_and_the_limit_frames_are_what_the_issue_lists():
    frames = jen.many_frames()
    assert len(frames) == 300 and [f.shape[:2] for f in frames[:4]] == [(1, 1), (7, 7), (8, 9), (17, 23)]
    assert all(f.shape[:2] == jen.MANY_SIZES[i % 4] and f.dtype == np.uint8 for i, f in enumerate(frames))
    assert len({f.tobytes() for f in frames[3::4]}) == 75           # mixed content: no two of the largest alike
    assert jen.limit_frame(1, 65535).shape == (1, 65535, 3) and jen.limit_frame(65535, 1).shape == (65535, 1, 3)


def only_alphabet_reaches():
    """The lowest luma AC symbol that the alphabet case emits and no pixel fixture does."""
    _, ac = reached(NAMES)
    return min(meter("alphabet_420")["ac"][0] - ac[0])


def mutant_scan(name, mutant, arg=None):
    if name in CASES:
        c = CASES[name]
        return jen.scan_of(c["coef"], c["g"], c["restart"], mutant, arg), jen.coefficient_scan(name)
    g, coef, _ = jen.restated(name)
    return jen.scan_of(coef, g, FIX[name]["restart"], mutant, arg), jen.jec.scan_bytes(FIX[name]["jpeg"])


@pytest.mark.parametrize("mutant,arg,name", [
    ("dc11_as_dc10", None, "tiles_99x37_444"), ("dc11_as_dc10", None, "tiles_99x37_422"), ("dc11_as_dc10", None, "tiles_99x37_420"),
    ("dc11_as_dc10", None, "alphabet_420"), ("dc11_as_dc10", None, "alphabet_444"),
    ("ac_code", "only_alphabet", "alphabet_420"), ("ac_code", "only_alphabet", "alphabet_444"),
    ("no_align", 256, "tile_seam_422_r1"), ("no_align", 256, "tile_seam_422_r8"), ("no_align", 256, "tile_seam_422_r64"),
    ("no_align", 768, "tile_seam_420_r128"), ("no_align", 256, "seam_144x64_422"),
    ("final_ff_unstuffed", None, "ends_in_ff"), ("final_ff_unstuffed", None, "ends_in_ff_r1"),
    ("zrl_at_15", None, "alphabet_420"), ("zrl_at_15", None, "alphabet_444")])
def test_a_mutant_of_the_scan_coder_changes_the_bytes_of_its_case(mutant, arg, name):
    if arg == "only_alphabet":
        arg = only_alphabet_reaches()
        assert arg in jen.ALL_AC
    got, want = mutant_scan(name, mutant, arg)
    assert jen.scan_of(*((CASES[name]["coef"], CASES[name]["g"], CASES[name]["restart"]) if name in CASES else
                         (jen.restated(name)[1], jen.restated(name)[0], FIX[name]["restart"]))) == want      # the coder itself is right
    assert got != want


def test_the_older_fixtures_do_not_see_those_mutants():
    """Why the cases above are needed: the 59 older pixel fixtures pass a coder with a wrong DC category 11 or a wrong code
    for the symbol only the alphabet case reaches."""
    sym = only_alphabet_reaches()
    for n in [n for n in NAMES if n not in EDGES][::6]:
        assert mutant_scan(n, "dc11_as_dc10")[0] == mutant_scan(n, "ac_code", sym)[0] == jen.jec.scan_bytes(FIX[n]["jpeg"]), n


def test_the_debug_scan_checks_its_arguments_without_a_gpu():
    g = jen.geometry(23, 17, "4:2:0")
    good = np.zeros((g["total_blocks"], 64), np.int16)
    arrs, heights, widths, sub, ri = Engine._jpeg_scan_args([good, good[:6]], [(17, 23), (1, 1)], "4:2:0", 5)
    assert (heights, widths, sub, ri) == ([17, 1], [23, 1], 2, 5) and arrs[0].flags.c_contiguous
    assert Engine._jpeg_scan_args([], [], "4:4:4", 0)[0] == []
    with pytest.raises(ValueError, match="2 sizes for 1 coefficient"):
        Engine._jpeg_scan_args([good], [(17, 23), (17, 23)], "4:2:0", 0)
    for bad in (good.astype(np.int32), good.astype(np.float32), good.tolist(), None):
        with pytest.raises(ValueError, match="int16"):
            Engine._jpeg_scan_args([bad], [(17, 23)], "4:2:0", 0)
    for bad in (good[:-1], good.reshape(-1), good.reshape(-1, 32), good[:, :63]):
        with pytest.raises(ValueError, match=r"must be \(%d, 64\)" % g["total_blocks"]):
            Engine._jpeg_scan_args([bad], [(17, 23)], "4:2:0", 0)
    with pytest.raises(ValueError, match=r"must be \(27, 64\)"):     # the same blocks at another sampling
        Engine._jpeg_scan_args([good], [(17, 23)], "4:4:4", 0)
    with pytest.raises(ValueError, match="1..65535"):
        Engine._jpeg_scan_args([good], [(0, 23)], "4:2:0", 0)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        Engine._jpeg_scan_args([good], [(17, 23, 3)], "4:2:0", 0)
    with pytest.raises(ValueError, match="subsampling"):
        Engine._jpeg_scan_args([good], [(17, 23)], "420", 0)
    with pytest.raises(ValueError, match="restart_interval"):
        Engine._jpeg_scan_args([good], [(17, 23)], "4:2:0", -1)
    # the library's own checks in front of the device: a null handle and null arrays are refused
    L = _lib.lib()
    assert L.lwp_debug_jpeg_encode_scan(None, 1, None, None, None, 2, 0, None, None, None) == _lib.LWP_ERR_ARG
