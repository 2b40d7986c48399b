"""The small-M fp32 stage-head kernel (heads_f32_kernel: 32 pixels of ONE head of a merged pair per workgroup, the head's hidden
half split over 8 waves, two pixel blocks per weight fragment) through the C-ABI (-m gpu).

Shapes: M = 31 (one ragged workgroup per head), M = 32 (exactly one), M = 2 x 12 x 19 = 456 (ragged last tile, a tile that
straddles the two frames); both stages of a one-refinement network (hidden 2 x 512 and 2 x 128); head widths 19 + 38 and two
non-default splits (17 + 30: output tile 1 straddles the heads; 16 + 40: the split sits on a tile boundary).

Bounds (not restated, not loosened):
  * against the two GEMM launches (LWP_FUSE_HEADS=0) and the un-merged graph (LWP_MERGE_HEADS=0): NET_TOL of
    tests/test_gpu_parity.py, as test_fp32_fused_head_pair_matches_the_two_gemm_form uses it;
  * against the float64 oracle: F32_STAGE_TOL x rms of the reference map, the bound tests/test_kernel_variants.py puts on the
    heads_f32 row's stage outputs."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine
from oracle import net_ref

from test_gpu_parity import NET_TOL, net_input
from test_kernel_variants import F32_STAGE_TOL

pytestmark = pytest.mark.gpu

# (N, H, W) -> stride-8 maps of M pixels
FRAMES = {31: (1, 8, 248), 32: (1, 8, 256), 456: (2, 91, 149)}
WIDTHS = [(19, 38), (17, 30), (16, 40)]
SWITCHES = ("LWP_FUSE_HEADS", "LWP_MERGE_HEADS", "LWP_HEADS_F32_MAXM", "LWP_HEADS_F32_LDS")

_SD, _REF = {}, {}


def state_dict(nh, npaf):
    if (nh, npaf) not in _SD:
        _SD[(nh, npaf)] = synth.make_state_dict(1, seed=5, num_heatmaps=nh, num_pafs=npaf)
    return _SD[(nh, npaf)]


def frame(m):
    n, h, w = FRAMES[m]
    return net_input(n, h, w, seed=430 + m)


def ref64(m, nh, npaf):
    """float64 stage outputs of the oracle, computed once per shape and shared."""
    if (m, nh, npaf) not in _REF:
        outs = net_ref.forward64(state_dict(nh, npaf), torch.from_numpy(frame(m)), 1)
        _REF[(m, nh, npaf)] = [o.numpy() for o in outs]
    return _REF[(m, nh, npaf)]


def run(monkeypatch, m, nh, npaf, env):
    """Stage outputs (NCHW), the concat-buffer windows of the two `.heads.1` / `.pafs.1` layers and the variants recorded."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(0, nref=1, num_heatmaps=nh, num_pafs=npaf, dtype=_lib.F32)
    eng.load_state_dict(state_dict(nh, npaf))
    for k in env:
        monkeypatch.delenv(k)
    x = frame(m)
    outs = [np.asarray(o) for o in eng.forward(x)]
    heads = [l for l in eng.layers() if l["name"].endswith(".heads.1")]
    taps = {l["name"]: eng.debug_layer_output(x, l["index"]) for l in heads}
    var = {l["name"]: eng.layer_variant(l["index"]) for l in heads}
    again = [np.asarray(o) for o in eng.forward(x)]
    return outs, taps, var, again


@pytest.mark.parametrize("nh,npaf", WIDTHS, ids=["%d+%d" % w for w in WIDTHS])
@pytest.mark.parametrize("m", sorted(FRAMES))
def test_one_head_per_workgroup_form_against_two_gemms_unmerged_and_float64(monkeypatch, m, nh, npaf):
    ref = ref64(m, nh, npaf)
    fused, taps, var, again = run(monkeypatch, m, nh, npaf, {})
    plain, _, var_p, _ = run(monkeypatch, m, nh, npaf, {"LWP_FUSE_HEADS": "0"})
    unmerged, taps_u, _, _ = run(monkeypatch, m, nh, npaf, {"LWP_MERGE_HEADS": "0"})
    # the kernel under test ran both stages (initial: hidden 2 x 512, refinement: 2 x 128); the A/B engines did not
    assert sorted(var) == ["initial_stage.heads.1", "refinement_stages.0.heads.1"] and set(var.values()) == {"heads_f32<8>"}, var
    assert not any(v.startswith("heads_f32") for v in var_p.values()), var_p
    assert not taps_u                                            # the un-merged graph has no pair to fuse
    assert [o.shape[1] for o in fused] == [nh, npaf, nh, npaf]
    n, h, w = FRAMES[m]
    assert fused[0].shape[0] * fused[0].shape[2] * fused[0].shape[3] == m
    for i, (f, q, u, r) in enumerate(zip(fused, plain, unmerged, ref)):
        d = float(np.abs(f.astype(np.float64) - r).max())
        rms = float(np.sqrt(np.mean(r * r)))
        sc = max(1.0, float(np.abs(r).max()))
        print("M=%d %d+%d out %d: vs float64 %.3e (bound %.3e = F32_STAGE_TOL x rms %.4f), vs two GEMMs %.3e, vs un-merged %.3e"
              % (m, nh, npaf, i, d, F32_STAGE_TOL * rms, rms, float(np.abs(f - q).max()), float(np.abs(f - u).max())))
        assert d <= F32_STAGE_TOL * rms, (i, d, rms)
        assert np.abs(f - q).max() <= NET_TOL * sc and np.abs(f - u).max() <= NET_TOL * sc, i
    # every channel of the NHWC concat-buffer window equals its NCHW plane bit for bit: each workgroup wrote exactly its own
    # head's channels, in both layouts
    for k, nm in enumerate(("initial_stage.heads.1", "refinement_stages.0.heads.1")):
        assert taps[nm].shape[1] == nh + npaf
        assert np.array_equal(taps[nm][:, :nh], fused[2 * k]) and np.array_equal(taps[nm][:, nh:], fused[2 * k + 1]), nm
    # fixed reduction order: a second run on the same input is bit-identical
    for a, b in zip(fused, again):
        assert np.array_equal(a, b)
