"""GPU: the entropy stages of the JPEG encoder (stages B .. F of csrc/jpeg_encode_kernels.hip) on coefficients that
pixels do not reach, through lwp_debug_jpeg_encode_scan, against the reference scan coder (tests/jpeg_entropy_cases.py, pinned to
Pillow's files), byte for byte: every symbol of Annex K's four tables, blocks at the longest code the planner sizes for, restart
intervals that start on a tile seam of the offset scan, scans that end in 0xFF, interval starts on a chunk boundary, blocks
of six bits; then the limits of the API from pixels (300 images in one call, frames 65535 wide and high), the two debug
entries composed to the product path, the refusal of a coefficient outside the contract, and what a closed engine gives back.
test_jpeg_encode_host.py holds the cases to their conditions without a GPU."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine

import jpeg_encode_cases as jen
import jpeg_entropy_cases as jec

pytestmark = pytest.mark.gpu
FIX = jen.fixtures()
CASES = jen.coefficient_cases()
NAMES = sorted(CASES)
EDGES = sorted(n for n in FIX if n.startswith(("tiles_", "seam_")))
WORST = [n for n in NAMES if n.startswith("worst_")]


@pytest.fixture(scope="module")
def eng():
    return Engine(0, nref=1, num_channels=32)          # the encoder needs no weights


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def same(got, want, what):
    assert isinstance(got, bytes)
    assert got == want, "%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first_difference(got, want))


def scan_call(eng, names):
    c = [CASES[n] for n in names]
    return eng.debug_jpeg_encode_scan([x["coef"] for x in c], [x["size"] for x in c], c[0]["sampling"], c[0]["restart"])


def settings():
    """{(sampling, restart): [names]}: a call has one setting."""
    out = {}
    for n in NAMES:
        out.setdefault((CASES[n]["sampling"], CASES[n]["restart"]), []).append(n)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_each_coefficient_case_alone_equals_the_reference_scan(eng, name):
    got = scan_call(eng, [name])
    assert len(got) == 1
    same(got[0], jen.coefficient_scan(name), name)


@pytest.mark.parametrize("key", sorted(settings()))
def test_the_cases_of_a_setting_in_one_call_forward_and_reversed(eng, key):
    """Sizes from 3 to 864 blocks in one call: image boundaries fall inside the workgroups of stages B, D and F."""
    names = settings()[key]
    for order in (names, names[::-1]):
        for n, got in zip(order, scan_call(eng, order)):
            same(got, jen.coefficient_scan(n), "%s in %s" % (n, order))
    assert max(len(v) for v in settings().values()) >= 4


@pytest.mark.parametrize("name", WORST)
def test_worst_fits_the_bound_and_leaves_its_neighbour_alone(eng, name):
    c = CASES[name]
    H, W = c["size"]
    want = jen.coefficient_scan(name)
    other = jec.random_coefficients(7, c["g"], density=0.3, dc=500)
    # the neighbour stands behind the worst image in every region of the workspace, and in front of the next one
    got = eng.debug_jpeg_encode_scan([c["coef"], other, c["coef"], other], [c["size"]] * 4, c["sampling"], c["restart"])
    assert len(got[0]) == len(want)
    header = Engine.debug_jpeg_encode_header(H, W, 75, c["sampling"], c["restart"])
    assert len(got[0]) + len(header) + 2 <= Engine.jpeg_encode_bound(H, W, c["sampling"], c["restart"])
    same(got[0], want, name)
    same(got[2], want, name + " again")
    quiet = jen.scan_of(other, c["g"], c["restart"])
    same(got[1], quiet, "the neighbour of " + name)
    same(got[3], quiet, "the second neighbour of " + name)


def test_300_images_in_one_call_from_pixels(eng):
    frames = jen.many_frames()
    assert len(frames) == 300 > 256
    for quality, sampling, restart in ((75, "4:2:0", 0), (95, "4:2:2", 1)):
        got = eng.encode_jpeg_batch(frames, quality, sampling, restart)
        assert len(got) == 300
        for i, (f, data) in enumerate(zip(frames, got)):
            g, coef, _ = jen.forward_blocks(f, sampling, quality)
            header = Engine.debug_jpeg_encode_header(f.shape[0], f.shape[1], quality, sampling, restart)
            same(data, header + jen.scan_of(coef, g, restart) + b"\xff\xd9", "image %d" % i)


@pytest.mark.parametrize("height,width,sampling", [(1, 65535, "4:2:0"), (65535, 1, "4:2:2")])
def test_a_frame_at_the_dimension_limit(eng, height, width, sampling):
    frame = jen.limit_frame(height, width)
    g, coef, _ = jen.forward_blocks(frame, sampling, 75)
    for restart in (0, 1):
        got = eng.encode_jpeg_batch([frame], 75, sampling, restart)
        header = Engine.debug_jpeg_encode_header(height, width, 75, sampling, restart)
        same(got[0], header + jen.scan_of(coef, g, restart) + b"\xff\xd9", "%d x %d restart %d" % (height, width, restart))
        assert Engine.jpeg_info(got[0][:len(header)])["total_blocks"] == g["total_blocks"]
        if restart:
            assert got[0].count(b"\xff\xd7") >= g["mcus_x"] * g["mcus_y"] // 8 - 1      # thousands of intervals


def test_the_two_debug_entries_compose_to_the_product_path(eng):
    assert len(EDGES) == 6
    for n in EDGES:
        f = FIX[n]
        coefs, _ = eng.debug_jpeg_encode_blocks([torch.from_numpy(f["bgr"]).cuda()], f["quality"], f["sampling"])
        _, want, _ = jen.restated(n)
        assert int((coefs[0] != want).sum()) == 0, n
        got = eng.debug_jpeg_encode_scan(coefs, [f["bgr"].shape[:2]], f["sampling"], f["restart"])
        same(got[0], jec.scan_bytes(f["jpeg"]), n)


def scan_into(eng, coefs, sizes, sampling, restart, caps):
    n = len(coefs)
    ptrs = (ctypes.c_void_p * n)(*[c.ctypes.data for c in coefs])
    heights = (ctypes.c_int * n)(*[s[0] for s in sizes])
    widths = (ctypes.c_int * n)(*[s[1] for s in sizes])
    outs = [np.full(c, 7, dtype=np.uint8) for c in caps]
    optr = (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs])
    lens = (ctypes.c_size_t * n)()
    rc = _lib.lib().lwp_debug_jpeg_encode_scan(eng.h.ptr, n, ptrs, heights, widths, sampling, restart, optr, (ctypes.c_size_t * n)(*caps), lens)
    return rc, _lib.lib().lwp_last_error(eng.h.ptr).decode(), outs, [int(v) for v in lens]


def test_a_coefficient_outside_the_contract_is_refused_with_its_image(eng):
    g = jen.geometry(23, 17, "4:2:0")
    good = [jec.random_coefficients(s, g, density=0.2, dc=1000) for s in (1, 2, 3)]
    want = [jen.scan_of(c, g, 2) for c in good]
    caps = [Engine.jpeg_encode_bound(17, 23, "4:2:0", 2)] * 3
    for block, k, value in ((3, 5, 1024), (0, 0, 1024), (g["total_blocks"] - 1, 63, -1024), (2, 0, -1025)):
        bad = good[1].copy()
        bad[block, k] = value
        rc, msg, outs, _ = scan_into(eng, [good[0], bad, good[2]], [(17, 23)] * 3, 2, 2, caps)
        assert rc == _lib.LWP_ERR_ARG and msg.startswith("image 1: ") and str(value) in msg, msg
        assert all(bool((o == 7).all()) for o in outs)              # nothing is written
    edge = good[1].copy()
    edge[0, 0], edge[1, 0], edge[0, 1], edge[0, 2] = -1024, 1023, 1023, -1023          # the ends of the contract are inside it
    rc, msg, outs, lens = scan_into(eng, [good[0], edge, good[2]], [(17, 23)] * 3, 2, 2, caps)
    assert rc == _lib.LWP_OK, msg
    assert [o[:n].tobytes() for o, n in zip(outs, lens)] == [want[0], jen.scan_of(edge, g, 2), want[2]]
    # a capacity one byte short in the middle: its index, and nothing written; then exactly enough
    sizes = [len(w) for w in want]
    rc, msg, outs, _ = scan_into(eng, good, [(17, 23)] * 3, 2, 2, [sizes[0], sizes[1] - 1, sizes[2]])
    assert rc == _lib.LWP_ERR_CAPACITY and msg.startswith("image 1: ") and str(sizes[1]) in msg, msg
    assert all(bool((o == 7).all()) for o in outs)
    rc, msg, outs, lens = scan_into(eng, good, [(17, 23)] * 3, 2, 2, sizes)
    assert rc == _lib.LWP_OK and lens == sizes and [o.tobytes() for o in outs] == want
    with pytest.raises(ValueError, match="image 1: .*1..65535"):
        eng._call("lwp_debug_jpeg_encode_scan", 2, (ctypes.c_void_p * 2)(good[0].ctypes.data, good[0].ctypes.data), (ctypes.c_int * 2)(17, 0),
                  (ctypes.c_int * 2)(23, 23), 2, 0, (ctypes.c_void_p * 2)(), (ctypes.c_size_t * 2)(), (ctypes.c_size_t * 2)())
    assert eng.debug_jpeg_encode_scan([], []) == []
    assert eng.debug_jpeg_encode_scan(good, [(17, 23)] * 3, "4:2:0", 2) == want      # the engine is fine afterwards


def test_a_closed_engine_has_given_back_what_the_debug_scan_took():
    gc.collect()
    base = live()
    e = Engine(0, nref=1, num_channels=32)
    try:
        created = live()
        names = ["tile_seam_422_r8", "tile_seam_422_r8"]
        got = scan_call(e, names)
        grown = live()
        assert grown[0] > created[0] and grown[1] > created[1]          # the workspace and the pinned staging are counted
        assert scan_call(e, names) == got == [jen.coefficient_scan(names[0])] * 2
        assert live() == grown                                          # a second call of the same size takes nothing more
    finally:
        e.h.close()
    assert live() == base
