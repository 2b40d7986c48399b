"""CPU: the float64 network oracle (``net_ref.forward64``) that tests/test_kernel_variants.py measures the kernels against.

Pinned to the fp32 oracle and to the reference goldens (tests/golden/net_small_nref{1,3}.npz) within 1e-5 * scale: the same
straight-line forward, only the precision differs.  Also: ``stop_after`` ends the forward at a tap with the same values."""
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth
from oracle import net_ref

from conftest import GOLDEN

F64_PIN = 1e-5


def net_input(n, h, w, seed):
    fr = synth.make_frames(n, h, w, seed0=seed)
    x = (fr.astype(np.float32) - 128.0) * np.float32(1 / 256)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


@pytest.mark.parametrize("nref", [1, 3])
def test_float64_oracle_pinned_to_fp32_oracle_and_reference_goldens(nref):
    g = np.load(os.path.join(GOLDEN, "net_small_nref%d.npz" % nref))
    sd = synth.make_state_dict(nref, seed=1)
    x = torch.from_numpy(net_input(2, 64, 96, seed=100))
    t32, t64 = {}, {}
    o32 = net_ref.forward(sd, x, nref, t32)
    o64 = net_ref.forward64(sd, x, nref, t64)
    assert all(o.dtype == torch.float64 for o in o64) and all(t.dtype == torch.float64 for t in t64.values())
    assert set(t64) == set(t32) and len(o64) == len(o32) == 2 * (1 + nref)
    worst = 0.0
    for k in t32:
        a, b = t64[k].numpy(), t32[k].numpy().astype(np.float64)
        sc = max(1.0, float(np.abs(a).max()))
        err = float(np.abs(a - b).max())
        worst = max(worst, err / sc)
        assert err <= F64_PIN * sc, (k, err, sc)
    # the two precisions really differ (the cast took): fp32 rounding is visible at this depth
    assert worst > 1e-8
    for i, (a, b) in enumerate(zip(o64, o32)):
        assert np.abs(a.numpy() - b.numpy()).max() <= F64_PIN
        assert np.abs(a.numpy() - g["out%d" % i]).max() <= F64_PIN
    checked = 0
    for k in g.files:
        if k.startswith("tap:") and k[4:] in t64:
            ref = g[k].astype(np.float64)
            assert np.abs(t64[k[4:]].numpy().reshape(-1)[::7] - ref).max() <= F64_PIN * max(1.0, float(np.abs(ref).max())), k
            checked += 1
    assert checked >= 15 + 5 * nref


def test_float64_cast_keeps_integer_entries_and_input():
    sd = synth.make_state_dict(1, seed=1)
    x = net_input(1, 32, 48, seed=3)
    sd64, x64 = net_ref.to_float64(sd, x)
    assert x64.dtype == torch.float64 and np.array_equal(x64.numpy(), x.astype(np.float64))
    for k, v in sd.items():
        if v.is_floating_point():
            assert sd64[k].dtype == torch.float64 and torch.equal(sd64[k], v.double()), k
        else:
            assert sd64[k].dtype == v.dtype and torch.equal(sd64[k], v), k
    assert sd["model.0.0.weight"].dtype == torch.float32        # the caller's state dict is untouched


def test_stop_after_ends_at_the_named_tap_with_the_same_values():
    sd = synth.make_state_dict(1, seed=1)
    x = torch.from_numpy(net_input(1, 40, 56, seed=5))
    full, part = {}, {}
    net_ref.forward64(sd, x, 1, full)
    assert net_ref.forward64(sd, x, 1, part, stop_after="model.3") is None
    assert list(part) == list(full)[:list(full).index("model.3") + 1]
    for k in part:
        assert torch.equal(part[k], full[k]), k
    # the extra taps the variant tests use exist and have the layer shapes
    for k in ("refinement_stages.0.trunk.0.initial", "refinement_stages.0.trunk.4.trunk.0", "initial_stage.heatmaps.0",
              "initial_stage.pafs.1", "refinement_stages.0.heatmaps.1"):
        assert k in full, k
    assert full["initial_stage.heatmaps.0"].shape[1] == 512 and full["refinement_stages.0.pafs.0"].shape[1] == 128
