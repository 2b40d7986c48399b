"""The exact-arithmetic fixtures of tests/exact_cases.py, checked on the CPU (-m "not gpu").

Every fixture x {fp32, bf16, fp16} x frame must satisfy the exactness condition on every element (the headroom table is
printed: run with -s); BatchNorm folds exactly; the input channels of every layer under test are pairwise distinct; the
float64 restatement agrees bit for bit with independent restatements that sum in other orders (torch f32 convs, torch f64
convs, the bf16 budget tool's emulation); and every fixture bites: truncation instead of round-to-nearest-even, one dropped
32-channel K block and two swapped weight rows each change the reference of the layer under test."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import exact_cases as ec
from conftest import ROOT
from oracle import net_ref

SHAPES = ec.FRAMES
BY_NREF = sorted({f["nref"] for f in ec.FIXTURES})


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_list_covers_every_conv_and_every_fused_group():
    singles = {f["convs"][0] for f in ec.FIXTURES if not f["joint"] and f["nref"] == 1}
    assert singles == set(ec._conv_keys(1)) and len(singles) == 57
    joint = {f["name"] for f in ec.FIXTURES if f["joint"]}
    assert len(joint) == 11 + 3 + 2 + 4 + 1, sorted(joint)
    assert any(f["nref"] == 3 and f["convs"][0].startswith("refinement_stages.1.") for f in ec.FIXTURES)
    assert len({f["name"] for f in ec.FIXTURES}) == len(ec.FIXTURES)


def test_frames_are_multiples_of_2_to_the_minus_8():
    for shape in SHAPES:
        x = ec.frame_of(shape)
        k = x.astype(np.float64) * 256
        assert x.dtype == np.float32 and x.shape == (shape[0], 3) + shape[1:]
        assert np.array_equal(k, np.round(k)) and k.min() == -128 and k.max() == 127


@pytest.mark.parametrize("nref", BY_NREF)
def test_selectors_have_one_weight_per_output_and_power_of_two_gains(nref):
    sd = ec.selector(nref)
    for key, v in sd.items():
        if key.endswith(".weight") and v.dim() == 4:
            w = v.numpy().reshape(v.shape[0], -1)
            assert np.all((w != 0).sum(axis=1) == 1), key
            g = w[w != 0]
            assert np.all(g > 0) and np.all(np.frexp(g)[0] == 0.5), key
        elif key.endswith(".bias") or key.endswith(".running_mean"):
            k = v.numpy().astype(np.float64) * 256
            assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 8, key


def test_batchnorm_folds_exactly():
    """float(w * gamma / sqrt((double)var + 1e-5)) is w * gamma, and the folded bias is (bias - mean) * gamma + beta, for every
    value the fixtures use and for k 2^-j (|k| <= 8, j <= 7) and biases k / 256 in general."""
    var = np.float64(ec.VAR)
    for gamma in (0.5, 1.0, 2.0, 4.0):
        sc = gamma / np.sqrt(var + 1e-5)
        assert abs(sc / gamma - 1) < 7e-9
        for j in range(8):
            for k in range(-8, 9):
                w = np.float32(k * 2.0 ** -j)
                assert np.float32(np.float64(w) * sc) == np.float32(np.float64(w) * gamma)
        for k in range(-1024, 1025):
            assert np.float32(np.float64(k / 256.0) * sc) == np.float32(k / 256.0 * gamma)
    for fx in ec.FIXTURES:
        sd = ec.dense_sd(fx)
        for conv in ec._conv_keys(fx["nref"]):
            bn = ec._bn_of(conv)
            if bn is None:
                continue
            w, b = ec.fold(sd, conv, bn)
            g = sd[bn + ".weight"].double()
            cb = sd[conv + ".bias"].double() if conv + ".bias" in sd else 0.0
            assert torch.equal(w, sd[conv + ".weight"].double() * g.view(-1, 1, 1, 1)), (fx["name"], conv)
            assert torch.equal(b, (cb - sd[bn + ".running_mean"].double()) * g + sd[bn + ".bias"].double()), (fx["name"], conv)


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_every_fixture_is_exact_on_every_element(shape, dtype):
    lo, hi = ec.NORMAL[dtype]
    bad = []
    print("\n%-46s %-5s %-9s %8s %8s %12s %12s" % ("fixture", "dtype", "frame", "own", "upto", "stored min", "stored max"))
    for fx in ec.FIXTURES:
        e = ec.fixture_exactness(fx, shape, dtype)
        print("%-46s %-5s %-9s %8.2f %8.2f %12.4g %12.4g" % (fx["name"], dtype, "x".join(map(str, shape)), e["own"], e["headroom"],
                                                             e["stored_min"], e["stored_max"]))
        if not (e["headroom"] > 0 and e["own"] > 0 and e["elu_min"] >= 0 and lo <= e["stored_min"] and e["stored_max"] <= hi):
            bad.append((fx["name"], e["headroom"], e["elu_min"], e["stored_min"], e["stored_max"]))
    assert not bad, bad


def _input_of(conv, ref):
    """The tensor a conv of the state dict reads, out of a reference() result."""
    p = conv.split(".")
    if p[0] == "model":
        i = int(p[1])
        if i == 0:
            return None
        return ref["model.%d.dw" % i] if p[2] == "3" else ref["model.0" if i == 1 else "model.%d.pw" % (i - 1)]
    if conv == "cpm.align.0":
        return ref["model.11.pw"]
    if p[0] == "cpm" and p[1] == "trunk":
        j = int(p[2])
        return ref["cpm.trunk.%d.dw" % j] if p[3] == "2" else ref["cpm.align" if j == 0 else "cpm.trunk.%d.pw" % (j - 1)]
    if conv == "cpm.conv.0":
        return ref["cpm.trunk.2.pw"]
    if p[0] == "initial_stage" and p[1] == "trunk":
        return ref["cpm.conv" if p[2] == "0" else "initial_stage.trunk.%d" % (int(p[2]) - 1)]
    if p[-3] in ("heatmaps", "pafs"):
        stage = ".".join(p[:-3])
        if p[-2] == "0":
            return ref["initial_stage.trunk.2" if stage == "initial_stage" else stage + ".trunk.4.trunk.1"]
        hid = ref[stage + ".heads.0"]
        half = hid.shape[1] // 2
        return hid[:, :half] if p[-3] == "heatmaps" else hid[:, half:]
    k, b = int(p[1]), int(p[3])
    q = "refinement_stages.%d.trunk.%d" % (k, b)
    if p[4] == "initial":
        if b > 0:
            return ref["refinement_stages.%d.trunk.%d.trunk.1" % (k, b - 1)]
        prev = "initial_stage" if k == 0 else "refinement_stages.%d" % (k - 1)
        return np.concatenate([ref["cpm.conv"], ref[prev + ".heads.1.cat"]], axis=1)
    return ref[q + ".initial"] if p[5] == "0" else ref[q + ".trunk.0"]


@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_input_channels_of_every_layer_under_test_are_pairwise_distinct(dtype):
    """Otherwise a permutation of K among equal channels would be invisible."""
    bad = []
    for shape in SHAPES:
        for fx in ec.FIXTURES:
            ref = ec.fixture_reference(fx, shape, dtype)
            for conv in fx["convs"]:
                xin = ec.frame_of(shape) if conv == "model.0.0" else _input_of(conv, ref)
                rows = np.ascontiguousarray(xin.transpose(1, 0, 2, 3)).reshape(xin.shape[1], -1)
                if len(np.unique(rows, axis=0)) != rows.shape[0]:
                    bad.append((fx["name"], conv, shape, len(np.unique(rows, axis=0)), rows.shape[0]))
    assert not bad, bad


def _net_ref_stop(layer):
    """oracle.net_ref tap after which the forward may end for engine layer ``layer``."""
    if layer.startswith("model.") and layer.endswith(".pw"):
        return layer[:-3]
    if layer == "cpm.conv":
        return "cpm"
    if layer.startswith("cpm.trunk."):
        return "cpm.sum" if layer == "cpm.trunk.2.pw" else layer[:-3]
    if layer.endswith(".heads.0") or layer.endswith(".heads.1"):
        return layer[:-len(".heads.0")] + ".pafs." + layer[-1]
    if layer.startswith("refinement_stages.") and layer.endswith(".trunk.1") and layer.count(".trunk.") == 2:
        return layer[:-len(".trunk.1")]
    return layer


def _f64_state(sd):
    """The state dict in float64 with running_var = the double for which var + 1e-5 is 1: torch's float64 BatchNorm then scales
    by exactly gamma (with the f32 variance it would be off by 7e-9, which the fold's rounding to f32 removes on the device)."""
    v = np.float64(1.0) - np.float64(1e-5)
    assert v + np.float64(1e-5) == 1.0
    return {k: (torch.full_like(t, v, dtype=torch.float64) if k.endswith(".running_var") else t.double() if t.is_floating_point() else t)
            for k, t in sd.items()}


@pytest.mark.parametrize("part", range(4))
def test_fp32_reference_equals_torch_f32_and_f64_restatements(part):
    """Order does not matter: oracle.net_ref in torch f32 (its own blocking and summation order, BatchNorm unfolded) and in
    float64 give the same bits as the float64 restatement, tap for tap, up to the layer under test."""
    shape = SHAPES[1]
    x = torch.from_numpy(ec.frame_of(shape))
    for fx in ec.FIXTURES[part::4]:
        sd = ec.dense_sd(fx)
        ref = ec.fixture_reference(fx, shape, "fp32")
        stop = _net_ref_stop(ec.last_layer(fx))
        t32, t64 = {}, {}
        net_ref.forward(sd, x, fx["nref"], t32, stop_after=stop)
        net_ref.forward(_f64_state(sd), x.double(), fx["nref"], t64, stop_after=stop)
        assert stop in t32 and stop in t64
        checked = 0
        for name, want in ref.items():
            if name.startswith("_") or name.endswith(".cat"):
                continue
            for taps in (t32, t64):
                try:
                    got = ec.tap_of(name, {k: v.numpy() for k, v in taps.items()})
                except KeyError:
                    continue                      # (a head pair's other half when the forward stopped in between)
                assert got.shape == want.shape and np.array_equal(got.astype(np.float64), want), (fx["name"], name)
                checked += 1
        assert checked >= 2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_head_references_equal_the_budget_emulation(dtype):
    """tools/bf16_budget.forward_emulated (torch f32 convs on rounded operands, every rounding group on; its rounding swapped
    to IEEE half as tests/test_gpu_f16.py does) gives the stage outputs of the head fixtures bit for bit."""
    bb = _tool("f16_budget")._budget()
    if dtype == "fp16":
        bb.rb = lambda t: t.to(torch.float16).to(torch.float32)
    shape = SHAPES[0]
    x = torch.from_numpy(ec.frame_of(shape))
    heads = [f for f in ec.FIXTURES if f["nref"] == 1 and ec.last_layer(f).endswith(".heads.1")]
    assert len(heads) >= 6
    for fx in heads:
        sd = ec.dense_sd(fx)
        ref = ec.reference(sd, x, 1, dtype, base=ec.selector_run(shape, dtype))
        outs = bb.forward_emulated(sd, x, 1, set(bb.GROUPS))
        for stage, (h, p) in (("initial_stage", outs[0:2]), ("refinement_stages.0", outs[2:4])):
            got = np.concatenate([h.numpy(), p.numpy()], axis=1).astype(np.float64)
            assert np.array_equal(got, ref[stage + ".heads.1"]), (fx["name"], stage)


def _mutations(fx, conv, sd):
    """(what, state dict) with one fault in the dense weights of ``conv``."""
    w = sd[conv + ".weight"]
    co, cig = w.shape[0], w.shape[1]
    out = []
    z = w.clone()
    if cig >= 32:
        b = (co + cig) % (cig // 32)
        z[:, 32 * b:32 * b + 32] = 0                    # one 32-channel K block
    elif cig == 3:
        z[:, 1] = 0                                     # the stem: one of its three input channels
    else:
        b = co % max(1, co // 32)
        z[32 * b:32 * b + 32] = 0                       # depthwise: K is the taps; 32 channels lose theirs
    out.append(("K block dropped", z))
    s = w.clone()
    r0, r1 = 1, co - 2
    s[[r0, r1]] = w[[r1, r0]]
    out.append(("rows swapped", s))
    for what, t in out:
        m = dict(sd)
        m[conv + ".weight"] = t
        yield what, m


@pytest.mark.parametrize("dtype", ec.DTYPES)
def test_every_fixture_bites(dtype):
    shape = SHAPES[0]
    bad = []
    for fx in ec.FIXTURES:
        keys = [l + ".cat" if dtype != "fp32" and l.endswith(".heads.1") else l for l in fx["layers"]]
        sd = ec.dense_sd(fx)

        def same(ref, good):
            return all(np.array_equal(ref[k], good[k]) for k in keys)
        good = ec.fixture_reference(fx, shape, dtype)
        if dtype != "fp32":
            if same(ec.fixture_reference(fx, shape, dtype, rounding="truncate"), good):
                bad.append((fx["name"], "truncation"))
        for conv in fx["convs"]:
            for what, bad_sd in _mutations(fx, conv, sd):
                assert not torch.equal(bad_sd[conv + ".weight"], sd[conv + ".weight"]), (fx["name"], conv, what)
                if same(ec.fixture_reference(fx, shape, dtype, sd=bad_sd), good):
                    bad.append((fx["name"], conv, what))
    assert not bad, bad
