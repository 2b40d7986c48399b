"""The lean form of the two-phase fused kernel ``dwpw_kernel<16,16>`` against the classic body of the same library,
bit for bit (-m gpu).

The lean form (``LWP_DWPW_LEAN=1``) walks the depthwise phase in row steps so that fewer registers are live at once; it moves
no arithmetic: every depthwise output keeps its chain ``acc = bias; acc += win * w`` for the nine taps in tap order, and the
K loop and the epilogue are the classic ones.  ``LWP_DWPW_LEAN=0`` runs the classic ``<16,16>`` body and is the reference
here, so no fixture file is needed.  Both engines must report ``dwpw<16,16>``, and a second run must equal the first.

Layers: model.6.pw (C = 256: half of the threads have no depthwise item), model.7.pw (dilation 2: only the general path),
model.8.pw (512 -> 512, dilation 1: the window fast path).  Frames are those of tests/gemm_ar_cases.py: an odd-width 12 x 19
map over two frames (pixel pairs straddle row ends, tiles straddle the frames, ragged last tile), a 1 x 32 map (every dy != 0
tap is outside) and a 3 x 5 map (less than one tile; dilation 2 reaches outside on every side)."""
import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine

import gemm_ar_cases as gc

pytestmark = pytest.mark.gpu

LAYERS = ["model.6.pw", "model.7.pw", "model.8.pw"]
FRAMES = [gc.BIG] + gc.SMALL

_CACHE = {}


def frame_input(frame):
    if frame not in _CACHE:
        n, h, w = frame
        x = (synth.make_frames(n, h, w, seed0=400).astype(np.float32) - 128.0) * np.float32(1 / 256)
        _CACHE[frame] = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    return _CACHE[frame]


def engine(monkeypatch, lean):
    """One engine per value of the switch (read once, at creation), shared by the frames."""
    if ("eng", lean) not in _CACHE:
        if "sd" not in _CACHE:
            _CACHE["sd"] = synth.make_state_dict(1, seed=1)
        for k in ("LWP_DWPW_BM", "LWP_DWPW_NW", "LWP_DWPW_PIPE", "LWP_DWPW_DEBUG", "LWP_FUSE_DWPW"):
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("LWP_DWPW_LEAN", lean)
        eng = Engine(0, nref=1, dtype=_lib.F32)
        eng.load_state_dict(_CACHE["sd"])
        _CACHE[("eng", lean)] = eng
    return _CACHE[("eng", lean)]


@pytest.mark.parametrize("frame", FRAMES, ids=["%dx%dx%d" % f for f in FRAMES])
def test_lean_keeps_every_bit_of_the_classic_body(monkeypatch, frame):
    classic, lean = engine(monkeypatch, "0"), engine(monkeypatch, "1")
    x = frame_input(frame)
    idx = {l["name"]: l["index"] for l in lean.layers()}
    for nm in LAYERS:
        want = classic.debug_layer_output(x, idx[nm])
        assert classic.layer_variant(idx[nm]) == "dwpw<16,16>", (nm, classic.layer_variant(idx[nm]))
        got = lean.debug_layer_output(x, idx[nm])
        assert lean.layer_variant(idx[nm]) == "dwpw<16,16>", (nm, lean.layer_variant(idx[nm]))
        again = lean.debug_layer_output(x, idx[nm])
        assert got.dtype == np.float32 and got.shape == want.shape, (nm, got.shape, want.shape)
        assert np.isfinite(want).all() and float(np.abs(want).max()) > 0, nm
        a, b, w = got.view(np.uint32), again.view(np.uint32), want.view(np.uint32)
        assert np.array_equal(a, b), (nm, "second run differs", int((a != b).sum()))
        bad = np.argwhere(a != w)
        assert bad.size == 0, (nm, "%d of %d values differ" % (len(bad), a.size), "first at %s: %r != %r" % (
            tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))
