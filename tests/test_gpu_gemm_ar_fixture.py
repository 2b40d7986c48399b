"""The A-resident f32 GEMM convs (``gemm_ar_kernel``) against tests/golden/gemm_ar_layers.npz, bit for bit (-m gpu).

The fixture was recorded by tools/record_gemm_layers.py on the commit before the kernel's prologue and epilogue were
re-ordered (loads issued back to back at entry, compile-time dilation, buffer loads / stores in the epilogue).  That change
moves no arithmetic: every accumulator receives the same MFMAs in the same order and the split-K sum keeps its order
0, 1, ..., KS - 1, so every output must keep every bit — at frames chosen for the index and bounds logic (tests/gemm_ar_cases.py):
a map narrower than a window segment, a one-row map, a map smaller than one tile; default engine and the forced forms that
share the template (uneven K groups, several blocks per group, groups without blocks, cout 57 < cout_pad 64 with the NCHW split).
Each layer is run twice and the second run must equal the first."""
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine

import gemm_ar_cases as gc

pytestmark = pytest.mark.gpu

_CACHE = {}


def fixture(golden_dir):
    if "fx" not in _CACHE:
        _CACHE["fx"] = gc.unpack(np.load(os.path.join(golden_dir, "gemm_ar_layers.npz")))
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
        for k in gc.SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = Engine(0, nref=1, dtype=_lib.F32)
        eng.load_state_dict(state_dict())
        _CACHE[("eng", cfg)] = eng
    return _CACHE[("eng", cfg)]


CASES = gc.cases()


def test_fixture_holds_every_case(golden_dir):
    want, variants = fixture(golden_dir)
    keys = {gc.key(fr, cfg, nm) for fr, cfg, _env, layers in CASES for nm in layers}
    assert set(want) == keys and set(variants) == keys
    assert all(v.startswith("gemm_ar<") for v in variants.values()), sorted(set(variants.values()))
    # the forms the table promises: every forced configuration, both kernel sizes, and the heuristic's own picks
    seen = set(variants.values())
    for c in gc.FORCED:
        bn, ks = c.split(",")[1:]
        assert {"gemm_ar<%s,%s,1>" % (bn, ks), "gemm_ar<%s,%s,3>" % (bn, ks)} <= seen, c


@pytest.mark.parametrize("frame,cfg,env,layers", CASES, ids=["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in CASES])
def test_layers_keep_every_bit(monkeypatch, golden_dir, frame, cfg, env, layers):
    want, variants = fixture(golden_dir)
    eng = engine(monkeypatch, cfg, env)
    x = frame_input(frame)
    idx = {l["name"]: l["index"] for l in eng.layers()}
    for nm in layers:
        k = gc.key(frame, cfg, nm)
        got = eng.debug_layer_output(x, idx[nm])
        assert eng.layer_variant(idx[nm]) == variants[k], (k, eng.layer_variant(idx[nm]), variants[k])
        again = eng.debug_layer_output(x, idx[nm])
        assert got.dtype == np.float32 and got.shape == want[k].shape, (k, got.shape, want[k].shape)
        a, b, w = got.view(np.uint32), again.view(np.uint32), want[k].view(np.uint32)
        assert np.array_equal(a, b), (k, "second run differs", int((a != b).sum()))
        bad = np.argwhere(a != w)
        assert bad.size == 0, (k, "%d of %d values differ" % (len(bad), a.size), "first at %s: %r != %r" % (
            tuple(bad[0]), float(got[tuple(bad[0])]), float(want[k][tuple(bad[0])])))
