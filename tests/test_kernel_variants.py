"""Every kernel variant of tests/variant_matrix.py forced on the GPU and compared with the float64 oracle (-m gpu).

Per row: an engine is created with the row's LWP_* switches (read once per handle at lwp_create), the row's layers are run
through ``debug_layer_output`` and each must record the row's exact ``layer_variant()`` string (the switch took).  Then:
  * fp32: every target layer within F32_TOL * max(1, max|ref64|) of the float64 tap; stage outputs within F32_STAGE_TOL * rms;
  * bf16: the documented BF16_TOL / BF16_MEAN against the float64 tap;
  * same input, other kernel: at the first layer whose variant differs from the baseline engine's (same structural switches,
    default kernels), both engines read bit-identical inputs, so the outputs may differ by summation order only —
    F32_SAME * scale in fp32, one bf16 rounding step per element in bf16 (bit-identical where the arithmetic is the same);
  * up-sample kernels and the fused multi-scale step at forced tile widths: bit-exact against oracle/post_ref.

The bounds were set from the worst errors measured over all rows on an MI355X (about 4x headroom); see the constants."""
import json
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine
from oracle import net_ref, post_ref

import variant_matrix as vm

pytestmark = pytest.mark.gpu

# Measured on an MI355X over all rows (worst err / scale): fp32 layers 2.3e-6 vs float64 (gemm_ar), stage outputs 8.3e-6 of
# the rms (heads_f32), same-input differences 1.2e-6 (gemm_ar<64,1,3> against <64,4,3>); bf16 same-input differences 2.8e-4
# (gemm_bf16_ar against gemm_bf16; every other bf16 variant is bit-identical to its default).  Bounds: about 4x those.
# fp32 vs float64, relative to max(1, max|ref|) (NET_TOL of tests/test_gpu_parity.py is 1e-3)
F32_TOL = 1e-5
# fp32 stage outputs (|ref| < 1, rms 0.05 - 0.15) vs float64, relative to the rms of the reference map
F32_STAGE_TOL = 3.5e-5
# fp32, same input, another kernel: summation order only
F32_SAME = 5e-6
# bf16, same input, another kernel: one bf16 rounding step (2^-7 relative) plus a small absolute term (scale-relative)
BF16_STEP = 2.0 ** -7
BF16_ABS = 1e-3
# bf16 vs float64 (the documented bf16 bounds of tests/test_gpu_parity.py)
BF16_TOL = 0.10
BF16_MEAN = 0.0105

# every kernel-choice switch a row may set: cleared before each engine so that one row's switch never leaks into another's
SWITCHES = sorted({k for r in vm.ROWS for k in r["env"]} | {k for u in vm.UPSAMPLE_ROWS for k in u["env"]} | {"LWP_MS_TX"})

REPORT = {"rows": [], "variants_seen": {}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("LWP_VARIANT_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


_SD = {}
_INPUT = {}
_REF64 = {}


def state_dict():
    if "sd" not in _SD:
        _SD["sd"] = synth.make_state_dict(1, seed=1)
    return _SD["sd"]


def frame_input(frame):
    if frame not in _INPUT:
        n, h, w = frame
        fr = synth.make_frames(n, h, w, seed0=400)
        x = (fr.astype(np.float32) - 128.0) * np.float32(1 / 256)
        _INPUT[frame] = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    return _INPUT[frame]


def ref64(frame, backbone_only):
    """float64 taps of the oracle for this input (large frames: up to model.3 only)."""
    key = (frame, backbone_only)
    if key not in _REF64:
        taps = {}
        net_ref.forward64(state_dict(), torch.from_numpy(frame_input(frame)), 1, taps, stop_after="model.3" if backbone_only else None)
        _REF64[key] = {k: v.numpy() for k, v in taps.items()}
    return _REF64[key]


def tap_of(name, taps):
    """float64 oracle activation that engine layer ``name`` writes."""
    if name.startswith("model.") and name.endswith(".pw"):
        return taps[name[:-3]]
    if name == "cpm.conv":
        return taps["cpm"]
    if name.startswith("cpm.trunk.") and name.endswith(".pw"):
        return taps["cpm.sum"] if name == "cpm.trunk.2.pw" else taps[name[:-3]]
    if name.endswith(".heads.0") or name.endswith(".heads.1"):
        p, k = name[:-len(".heads.0")], name[-1]
        return np.concatenate([taps[p + ".heatmaps." + k], taps[p + ".pafs." + k]], axis=1)
    if name.startswith("refinement_stages.") and name.endswith(".trunk.1") and name.count(".trunk.") == 2:
        return taps[name[:-len(".trunk.1")]]
    return taps[name]


def is_stage_output(name):
    return name.endswith(".heads.1") or name.endswith(".heatmaps.1") or name.endswith(".pafs.1")


def make_engine(monkeypatch, env, dtype):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(0, nref=1, dtype=_lib.BF16 if dtype == "bf16" else _lib.F32)
    eng.load_state_dict(state_dict())
    for k in env:
        monkeypatch.delenv(k)
    return eng


def run_layers(eng, x, names):
    """{name: output} for ``names`` and the variant every layer up to the last of them recorded."""
    idx = {l["name"]: l["index"] for l in eng.layers()}
    missing = [n for n in names if n not in idx]
    assert not missing, missing
    outs = {n: eng.debug_layer_output(x, idx[n]) for n in sorted(names, key=lambda n: idx[n])}
    last = max(idx[n] for n in names)
    eng.debug_layer_output(x, last)                       # one pass: every layer up to `last` records its variant
    order = sorted(idx, key=idx.get)[:last + 1]
    return outs, [(n, eng.layer_variant(idx[n])) for n in order]


_BASE = {}


def baseline(monkeypatch, row, x):
    """Engine with the row's structural switches only (every kernel choice at its default), cached per (switches, dtype, frame)."""
    env = {k: v for k, v in row["env"].items() if k in vm.STRUCTURAL}
    key = (tuple(sorted(env.items())), row["dtype"], row["frame"])
    if key not in _BASE:
        _BASE[key] = make_engine(monkeypatch, env, row["dtype"])
    return _BASE[key]


def _row_id(r):
    env = ",".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items()))
    return "%s-%s-%s-%s" % (r["dtype"], r["variant"], env or "default", r["layers"][0])


@pytest.mark.parametrize("row", vm.ROWS, ids=[_row_id(r) for r in vm.ROWS])
def test_forced_variant_against_float64_and_default(monkeypatch, row):
    x = frame_input(row["frame"])
    backbone_only = row["frame"] != vm.FRAME
    taps = ref64(row["frame"], backbone_only)
    eng = make_engine(monkeypatch, row["env"], row["dtype"])
    outs, seen = run_layers(eng, x, row["layers"])
    var = dict(seen)
    for nm in row["layers"]:
        REPORT["variants_seen"].setdefault(var[nm], [])
        if nm not in REPORT["variants_seen"][var[nm]]:
            REPORT["variants_seen"][var[nm]].append(nm)
    rec = dict(id=_row_id(row), family=row["family"], dtype=row["dtype"], layers={})
    REPORT["rows"].append(rec)
    # the switch took: every target layer ran the row's kernel
    assert {nm: var[nm] for nm in row["layers"]} == {nm: row["variant"] for nm in row["layers"]}, seen

    # against the float64 oracle
    for nm, got in outs.items():
        ref = tap_of(nm, taps)
        assert got.shape == ref.shape, (nm, got.shape, ref.shape)
        d = np.abs(got.astype(np.float64) - ref)
        scale = max(1.0, float(np.abs(ref).max()))
        rms = float(np.sqrt(np.mean(ref * ref)))
        rec["layers"][nm] = dict(max_rel=float(d.max()) / scale, mean_rel=float(d.mean()) / scale,
                                 stage_rel_rms=float(d.max()) / rms if is_stage_output(nm) else None)
        if row["dtype"] == "fp32":
            if is_stage_output(nm):
                assert d.max() <= F32_STAGE_TOL * rms, (nm, float(d.max()), rms)
            else:
                assert d.max() <= F32_TOL * scale, (nm, float(d.max()), scale)
        else:
            assert d.max() <= BF16_TOL * scale and d.mean() <= BF16_MEAN * scale, (nm, float(d.max()), float(d.mean()), scale)

    # against the default kernel on the same input: the first layer whose variant differs from the baseline engine's
    base = baseline(monkeypatch, row, x)
    _, bseen = run_layers(base, x, row["layers"])
    assert [n for n, _ in bseen] == [n for n, _ in seen]
    first = next((i for i, (a, b) in enumerate(zip(seen, bseen)) if a[1] != b[1]), None)
    if first is None:
        return                                            # the row's kernel is the default one here
    nm = seen[first][0]
    if nm.endswith(".heads.0") and first + 1 < len(seen) and seen[first + 1][1] == seen[first][1]:
        nm = seen[first + 1][0]                           # fused head pair: the hidden tensor is never written
    idx = {l["name"]: l["index"] for l in eng.layers()}
    a = eng.debug_layer_output(x, idx[nm]).astype(np.float64)
    b = base.debug_layer_output(x, idx[nm]).astype(np.float64)
    d = np.abs(a - b)
    scale = max(1.0, float(np.abs(b).max()))
    rec["same_input"] = dict(layer=nm, variant=var.get(nm), base_variant=dict(bseen).get(nm), max_rel=float(d.max()) / scale)
    if row["dtype"] == "fp32":
        assert d.max() <= F32_SAME * scale, (nm, float(d.max()), scale)
    else:
        assert np.all(d <= BF16_STEP * np.maximum(np.abs(a), np.abs(b)) + BF16_ABS * scale), (nm, float(d.max()), scale)


@pytest.mark.parametrize("row", vm.UPSAMPLE_ROWS, ids=["%s-x%d" % (u["kernel"], u["ratio"]) for u in vm.UPSAMPLE_ROWS])
def test_upsample_kernels_bit_exact(monkeypatch, row):
    """Per-element and tiled up-sample (x4, x8) on 19- and 38-channel maps whose up-sampled width is no multiple of the tile."""
    eng = make_engine(monkeypatch, row["env"], "fp32")
    heat, paf, _ = synth.make_pose_maps(3, 23, 41, 11)
    for m in (heat, paf):
        b = np.stack([m, m[::-1].copy()])
        got = eng.upsample(b, row["ratio"])
        for f in range(2):
            ref = post_ref.upsample_cubic(b[f].transpose(1, 2, 0), row["ratio"])
            assert got[f].shape == ref.shape
            assert np.array_equal(got[f], ref), (row, m.shape, f)


@pytest.mark.parametrize("tx", vm.MS_TX)
def test_multiscale_forced_tile_width_bit_exact(monkeypatch, tx):
    """Fused multi-scale step (x8 up-sample + crop + cubic resize + accumulate) at a forced tile width against the oracle."""
    eng = make_engine(monkeypatch, {"LWP_MS_TX": str(tx)}, "fp32")
    heat, paf, _ = synth.make_pose_maps(3, 23, 46, 21)
    for maps, pad, (dh, dw) in ((heat, [0, 3, 0, 3], (150, 301)), (paf, [20, 30, 12, 18], (184, 328))):
        acc0 = (synth.uniform((dh, dw, maps.shape[0]), 77) - 0.5).astype(np.float32)
        ref = post_ref.multiscale_accumulate(acc0.copy(), maps, 8, pad, dw, dh, 3)
        got = eng.multiscale_accumulate(np.ascontiguousarray(acc0.copy()), maps[None], 8, pad, 3)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (tx, maps.shape, pad, dh, dw)
