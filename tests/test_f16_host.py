"""LWP_F16 (fp16 storage of the conv stack) on the host side, no GPU: the dtype code at every layer, the channel widths the 16-bit
graph refuses, the weight packer's f32 -> fp16 rounding, and the CPU emulation that sets the fp16 bars of tests/test_gpu_f16.py."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet

from conftest import ROOT


def test_dtype_code_in_binding_and_header():
    assert _lib.F16 == 2 and _lib.BF16 == 1 and _lib.F32 == 0
    with open(os.path.join(ROOT, "include", "lwpose.h")) as f:
        hdr = f.read()
    assert re.search(r"\bLWP_F16\s*=\s*2\b", hdr)


@pytest.mark.parametrize("C_", [96, 160, 192, 32])
def test_create_refuses_widths_the_16bit_graph_cannot_run(C_):
    h = C.c_void_p()
    rc = _lib.lib().lwp_create(0, 1, C_, 19, 38, _lib.F16, C.byref(h))
    assert rc == _lib.LWP_ERR_ARG and not h.value
    assert "fp16 path supports" in _lib.lib().lwp_last_error(None).decode()


def test_model_wrapper_takes_fp16():
    net = PoseEstimationWithMobileNet(num_refinement_stages=1, dtype="fp16")
    assert net.dtype == _lib.F16
    bad = PoseEstimationWithMobileNet(num_refinement_stages=1, num_channels=96, dtype="fp16")
    with pytest.raises(ValueError, match="fp16 path supports"):
        bad.cuda()


def _host_f16(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.uint16)
    assert _lib.lib().lwp_debug_f32_to_f16(x.ctypes.data, out.ctypes.data, x.size) == 0
    return out


def _torch_f16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).half().view(torch.int16).numpy().view(np.uint16)


def test_host_rounding_equals_torch_half_bit_for_bit():
    # every finite fp16 value, the midpoints between neighbours (ties: round to even) and the f32 values just either side of them
    h = np.arange(0, 0x7C00, dtype=np.uint16)
    v = h.view(np.float16).astype(np.float32)
    mid = ((v[:-1].astype(np.float64) + v[1:]) / 2).astype(np.float32)             # exact in f32
    assert np.all(mid.astype(np.float64) == (v[:-1].astype(np.float64) + v[1:]) / 2)
    up, down = np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(0))
    top = np.array([65504, 65519.996, 65520, 65536, 1e5, 3.4e38, np.inf, 2 ** -24, 2 ** -25, 2 ** -26, 3 * 2 ** -26,
                    1.5 * 2 ** -25, 2 ** -14, 2 ** -14 - 2 ** -25, 0.0, 1e-45, 1e-40], dtype=np.float32)
    rng = np.random.default_rng(0)
    rnd = (rng.standard_normal(200000) * np.exp2(rng.uniform(-28, 18, 200000))).astype(np.float32)
    x = np.concatenate([v, mid, up, down, top, rnd])
    x = np.concatenate([x, -x])
    got, want = _host_f16(x), _torch_f16(x)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(float(x[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # subnormals and the overflow boundary are in there
    assert np.any((want & 0x7C00) == 0) and np.any(want == 0x7C00) and np.any(want == 0x7BFF)
    nan = _host_f16(np.array([np.nan, -np.nan], dtype=np.float32))
    assert np.all((nan & 0x7C00) == 0x7C00) and np.all(nan & 0x3FF)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_f16_emulation_meets_the_16bit_bar_on_one_frame():
    rows = _tool("f16_budget").measure(1, dtypes=("fp16",))
    r = rows["fp16"]
    for name, t in r["tensors"].items():
        assert t["max_abs_over_scale"] <= 0.01, (name, t)
        assert t["mean_abs_over_scale"] <= 0.0025, (name, t)
    assert r["oracle_kpts_matched"] >= 0.98 and r["emulated_kpts_matched"] >= 0.98, r
    for po, pe in r["poses_oracle_vs_emulated"]:
        assert abs(po - pe) <= 1
    assert r["largest_rounded"] < 65504 / 100          # far inside the fp16 range on this workload
