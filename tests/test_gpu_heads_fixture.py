"""The small-M fp32 stage-head pair (``heads_f32_kernel``) against tests/golden/heads_f32_layers.npz, bit for bit (-m gpu).

The fixture was recorded by tools/record_heads_layers.py on the commit before the kernel's memory side was re-ordered (no
weight request past the wave's last tile, the pixel tile loaded once per workgroup and handed to the waves through LDS, the
output bias requested at entry).  That change moves no arithmetic: every accumulator receives the same MFMAs in the same
order and the cross-wave sum keeps its order 0..7, so every output must keep every bit — at frames chosen for the index and
bounds logic (tests/heads_cases.py): exactly one pixel tile, a map smaller than one 16-pixel block, a ragged last tile with
tiles that straddle two frames; for the stage with four hidden tiles per wave (paired steps) and the one with a single tile
(the unpaired last step alone).  Both outputs of the pair are held: the NHWC window of the concat buffer and the NCHW stage
maps of an ordinary forward.  Everything is run twice and the second run must equal the first.

The LWP_MERGE_HEADS=0 configuration has no fused pair (four separate head convs, no ``.heads.1`` layer): its stage maps are
held too, but there is no ``heads_f32<8>`` launch in it to assert."""
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine

import heads_cases as hc

pytestmark = pytest.mark.gpu

_CACHE = {}


def fixture(golden_dir):
    if "fx" not in _CACHE:
        _CACHE["fx"] = hc.unpack(np.load(os.path.join(golden_dir, "heads_f32_layers.npz")))
    return _CACHE["fx"]


def state_dict():
    if "sd" not in _CACHE:
        _CACHE["sd"] = synth.make_state_dict(1, seed=1)
    return _CACHE["sd"]


def frame_input(frame):
    if frame not in _CACHE:
        n, h, w = frame
        x = (synth.make_frames(n, h, w, seed0=400).astype(np.float32) - 128.0) * np.float32(1 / 256)
        _CACHE[frame] = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    return _CACHE[frame]


def engine(monkeypatch, cfg, env):
    """One engine per configuration (the LWP_* switches are read once, at creation), shared by the frames."""
    if ("eng", cfg) not in _CACHE:
        for k in hc.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = Engine(0, nref=1, dtype=_lib.F32)
        eng.load_state_dict(state_dict())
        _CACHE[("eng", cfg)] = eng
    return _CACHE[("eng", cfg)]


def same_bits(k, got, again, want):
    assert got.dtype == np.float32 and got.shape == want.shape, (k, got.shape, want.shape)
    a, b, w = got.view(np.uint32), again.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(a, b), (k, "second run differs", int((a != b).sum()))
    bad = np.argwhere(a != w)
    assert bad.size == 0, (k, "%d of %d values differ" % (len(bad), a.size), "first at %s: %r != %r" % (
        tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))


CASES = hc.cases()


def test_fixture_holds_every_case(golden_dir):
    want, variants = fixture(golden_dir)
    keys = {hc.key(fr, cfg, w) for fr, cfg, _env, layers in CASES for w in layers + ["out%d" % i for i in range(hc.N_OUTS)]}
    assert set(want) == keys
    assert set(variants) == {hc.key(fr, cfg, nm) for fr, cfg, _env, layers in CASES for nm in layers}
    assert set(variants.values()) == {hc.VARIANT}


@pytest.mark.parametrize("frame,cfg,env,layers", CASES, ids=["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in CASES])
def test_head_outputs_keep_every_bit(monkeypatch, golden_dir, frame, cfg, env, layers):
    want, variants = fixture(golden_dir)
    eng = engine(monkeypatch, cfg, env)
    x = frame_input(frame)
    idx = {l["name"]: l["index"] for l in eng.layers()}
    assert all(nm in idx for nm in layers), layers
    for nm in layers:                                        # the NHWC window of the concat buffer
        k = hc.key(frame, cfg, nm)
        got = eng.debug_layer_output(x, idx[nm])
        assert eng.layer_variant(idx[nm]) == variants[k] == hc.VARIANT, (k, eng.layer_variant(idx[nm]))
        same_bits(k, got, eng.debug_layer_output(x, idx[nm]), want[k])
    first, second = eng.forward(x), eng.forward(x)           # the NCHW stage maps
    assert len(first) == hc.N_OUTS
    for i, (a, b) in enumerate(zip(first, second)):
        same_bits(hc.key(frame, cfg, "out%d" % i), a, b, want[hc.key(frame, cfg, "out%d" % i)])
