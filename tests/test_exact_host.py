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
    hi = ec.NORMAL[dtype][1]
    bad = []
    print("\n%-46s %-5s %-9s %8s %8s %12s %12s" % ("fixture", "dtype", "frame", "own", "upto", "stored min", "stored max"))
    for fx in ec.ALL_EXACT:
        lo = ec.NORMAL[dtype][0]
        e = ec.fixture_exactness(fx, shape, dtype)
        print("%-46s %-5s %-9s %8.2f %8.2f %12.4g %12.4g" % (fx["name"], dtype, "x".join(map(str, shape)), e["own"], e["headroom"],
                                                             e["stored_min"], e["stored_max"]))
        if fx.get("subnormal_ok") and dtype == "fp16":       # the f16sub fixtures: gradual underflow is what they are about
            lo = 2.0 ** -24
        if fx.get("nonfinite_ok"):                           # the f16ovf fixtures: inf at fp16 only; the consumer's reduction is
            assert (e["stored_max"] == np.inf) == (dtype == "fp16"), (fx["name"], dtype, e["stored_max"])      # measured per row
            e["stored_max"] = min(e["stored_max"], hi)
            own = _ovf_consumer_headroom(fx, shape, dtype)
            rest = [v for k, v in e["per_reduction"].items() if k.split("/")[0] != ec.last_layer(fx) or k.endswith("/res")]
            e["own"], e["headroom"] = min(own, e["own"]) if not fx["name"].endswith("heads>concat") else own, min(rest + [own])
        if not (e["headroom"] > 0 and e["own"] > 0 and e["elu_min"] >= 0 and lo <= e["stored_min"] and e["stored_max"] <= hi):
            bad.append((fx["name"], e["headroom"], e["elu_min"], e["stored_min"], e["stored_max"]))
    assert not bad, bad


def _ovf_consumer_headroom(fx, shape, dtype):
    """24 - bits of the consumer's reduction of an f16ovf fixture, per output row: one product of a finite input with a power
    of two plus the bias (the global measure compares the largest input of ANY channel with the smallest bit of any other)."""
    sd = ec.dense_sd(fx)
    up = fx["f16ovf"]["up"]
    ref = ec.fixture_reference(fx, shape, dtype)
    xin = _input_of(up, ref)
    w, b = ec.fold(sd, up, ec._bn_of(up))
    co, cig = w.shape[0], w.shape[1]
    w = w.numpy().reshape(co, -1)
    assert np.all((w != 0).sum(axis=1) == 1) and np.all(np.frexp(np.abs(w[w != 0]))[0] == 0.5)
    col = np.abs(w).argmax(axis=1)
    chan = np.arange(co) if cig == 1 and co > 3 else col // (w.shape[1] // cig)
    worst = 0.0
    for o in range(co):
        x = xin[:, chan[o]]
        x = x[np.isfinite(x) & (x != 0)]
        if x.size == 0:
            continue
        g = abs(w[o, col[o]])
        q = min(ec._lowbit(torch.from_numpy(x)) * g, ec._lowbit(b[o:o + 1]))
        worst = max(worst, float(np.log2((np.abs(x).max() * g + abs(float(b[o]))) / q)))
    return 24.0 - worst


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


# ------------------------------------------------------------------------------------------------------------ ELU below zero
def _elu_own_and_later(fx):
    j = fx["j"]
    own = "cpm.trunk.%d.%s" % (j, fx["elu"])
    later = ({"cpm.trunk.2.pw/res"} if j == 2 else set()) | ({"cpm.trunk.%d.pw" % j} if fx["elu"] == "dw" else set())
    return own, later


@pytest.mark.parametrize("dtype", ec.DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_elu_fixtures_sweep_an_exact_negative_operand(shape, dtype):
    """Per ELU fixture: z is exact (positive headroom on every reduction in front of it; its own reduction is one product of an
    f32 value with a power of two, no bias), every binade of |z| from 2^-22 to 2^6 holds at least 8 distinct operands (the
    .pw fixtures sit on the grid 2^-22, whose three lowest binades have 1, 2 and 4 points: all of them), both sides of the
    switch point -0.5 and the point itself, an operand below -104, zeros, and positive elements."""
    assert len(ec.ELU_FIXTURES) == 6 and not {f["name"] for f in ec.ELU_FIXTURES} & set(ec.BY_NAME)
    for fx in ec.ELU_FIXTURES:
        sd = ec.dense_sd(fx)
        ref = ec.elu_reference(fx, shape, dtype)
        own, later = _elu_own_and_later(fx)
        bits = {k: v for k, v in ref["_exact"].items() if not k.endswith("/elu_min")}
        assert own in bits and later <= set(bits)
        front = {k: v for k, v in bits.items() if k != own and k not in later}
        # the stem, 11 x 2, cpm.align, the trunk blocks in front
        assert len(front) >= 24 + 2 * fx["j"] and min(front.values()) > 0, (fx["name"], min(front, key=front.get))
        conv = fx["convs"][0]
        w = sd[conv + ".weight"].numpy().reshape(128, -1).astype(np.float64)
        assert conv + ".bias" not in sd and np.all((w != 0).sum(axis=1) == 1)
        g = w[w != 0]
        exps = ec.ELU_PW_EXP if fx["elu"] == "pw" else ec.ELU_DW_EXP
        assert np.all(np.frexp(np.abs(g))[0] == 0.5) and {float(v) for v in g} == {-2.0 ** e for e in exps} | {1.0}, fx["name"]
        if dtype != "fp32" and fx["elu"] == "pw":                # packed: a normal number of the format, unchanged by its rounding
            assert np.abs(g).min() >= ec.NORMAL[dtype][0] and np.array_equal(ec.ROUND[dtype](torch.from_numpy(g)).numpy(), g)
        xin = _input_of(conv, ref)
        own_bits = 24.0 - np.log2(np.abs(xin).max() / ec._lowbit(torch.from_numpy(xin)))
        assert own_bits > 0, (fx["name"], own_bits)
        # every ELU in front of the one under test stays on its identity branch
        for k, v in ref["_exact"].items():
            if k.endswith("/elu_min") and k[:-len("/elu_min")] not in (own, "cpm.trunk.%d.pw" % fx["j"]):
                assert v >= 0, (fx["name"], k, v)
        exp = ec.elu_expect(fx, ref, ec.last_layer(fx), dtype)
        z = exp["z"]
        a = np.unique(-z[exp["neg"]])
        lowest = -22 if fx["elu"] == "pw" else -30
        assert a.min() == 2.0 ** lowest, (fx["name"], a.min())
        for k in range(-22, 7):
            n = int(((a >= 2.0 ** k) & (a < 2.0 ** (k + 1))).sum())
            need = min(8, 2 ** (k + 22)) if fx["elu"] == "pw" else 8
            assert n >= need, (fx["name"], dtype, k, n)
        assert ((a > 0.5) & (a <= 0.5 + 2.0 ** -6)).any() and ((a < 0.5) & (a >= 0.5 - 2.0 ** -6)).any() and (a == 0.5).any(), fx["name"]
        assert (a > 104).any() and (z == 0).any() and (z > 0).any(), fx["name"]
        # the reference itself: expm1 in float64 where z < 0 (through the +-1 selector and the residual for the fused layer)
        if fx["j"] < 2 and fx["elu"] == "pw":
            want = np.where(z < 0, np.expm1(np.minimum(z, 0)), z)
            if dtype == "fp32":                                  # torch's float64 ELU and numpy's expm1: an ulp of float64 apart
                assert np.all(np.abs(exp["want"] - want) <= 2.0 ** -50 * np.abs(want)), fx["name"]
            else:
                assert np.array_equal(exp["want"], ec.ROUND[dtype](torch.from_numpy(want)).numpy()), fx["name"]
        assert np.all(exp["bound"][~exp["neg"]] == 0) and np.all(exp["bound"][exp["neg"]] > 0)
        assert np.all(((exp["want"] >= exp["lo"]) & (exp["want"] <= exp["hi"]))[exp["neg"]])


def _operands(fx, shape, dtype):
    exp = ec.elu_expect(fx, ec.elu_reference(fx, shape, dtype), "cpm.trunk.%d.%s" % (fx["j"], fx["elu"]), dtype)
    return np.unique(exp["z"][exp["z"] < 0])


@pytest.mark.parametrize("fx", ec.ELU_FIXTURES, ids=[f["name"] for f in ec.ELU_FIXTURES])
def test_elu_device_forms_restated_in_float32_meet_the_bounds(fx):
    """The polynomial / exp form of the fp32 kernels within 1e-6 relative of expm1, the exp(v) - 1 form of the 16-bit kernels
    within one step + 2^-22 of the rounded expm1, on every operand of the fixture (both frames)."""
    for shape in SHAPES:
        z = _operands(fx, shape, "fp32")
        e = np.expm1(z)
        err = np.abs(ec.elu_f32_form(z).astype(np.float64) - e)
        print("\n%s b%d fp32 form: worst error / bound %.3f (%d operands)" % (fx["name"], shape[0], float((err / (ec.ELU_F32_REL * np.abs(e))).max()), z.size))
        assert np.all(err <= ec.ELU_F32_REL * np.abs(e))
        for dtype in ("bf16", "fp16"):
            z = _operands(fx, shape, dtype)
            e = np.expm1(z)
            r = ec.ROUND[dtype]
            got = r(torch.from_numpy(ec.elu_cancelling_form(z).astype(np.float64))).numpy()
            err = np.abs(got - r(torch.from_numpy(e)).numpy())
            bound = ec.step16(dtype, e) + ec.ELU_16_ABS
            print("%s b%d %s form: worst error / bound %.3f" % (fx["name"], shape[0], dtype, float((err / bound).max())))
            assert np.all(err <= bound) and np.all(got <= 0) and np.all(got >= -1)


@pytest.mark.parametrize("fx", ec.ELU_FIXTURES, ids=[f["name"] for f in ec.ELU_FIXTURES])
def test_elu_bounds_bite_on_a_wrong_coefficient_a_moved_switch_and_the_cancelling_form(fx):
    shape = SHAPES[1]
    layer = "cpm.trunk.%d.%s" % (fx["j"], fx["elu"])
    exp = ec.elu_expect(fx, ec.elu_reference(fx, shape, "fp32"), layer, "fp32")
    z, neg = exp["z"], exp["neg"]
    res = exp["want"] - np.where(neg, np.expm1(np.minimum(z, 0)), z)            # the residual behind cpm.trunk.2.pw (else 0)

    def stored(form):
        v = np.where(neg, form(np.minimum(z, 0)).astype(np.float64), z) + res
        return v.astype(np.float32)
    bad, ratio = ec.elu_compare(stored(ec.elu_f32_form), exp)
    assert not bad and 0 < ratio <= 1, (bad, ratio)
    for what, form in ec.ELU_MUTANTS.items():
        bad, ratio = ec.elu_compare(stored(form), exp)
        assert bad and ratio > 1, (fx["name"], what, ratio)
    # and on the identity side: one bit of a positive element, a zero that is not zero
    got = stored(ec.elu_f32_form)
    at = tuple(np.argwhere(z > 0)[0])
    got[at] = np.nextafter(got[at], np.float32(0))
    assert ec.elu_compare(got, exp)[0]
    got = stored(ec.elu_f32_form)
    at = tuple(np.argwhere((z == 0) & (res == 0))[0]) if ((z == 0) & (res == 0)).any() else tuple(np.argwhere(z == 0)[0])
    got[at] -= np.float32(2.0 ** -24)
    assert ec.elu_compare(got, exp)[0]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("fx", ec.ELU_FIXTURES, ids=[f["name"] for f in ec.ELU_FIXTURES])
def test_elu_16bit_bound_bites_on_a_wrong_sign_a_lost_one_and_two_steps_but_not_on_truncation(fx, dtype):
    """How sharp step16 + 2^-22 is, on the restated exp(v) - 1 form followed by the 16-bit store.  Caught: exp(v) + 1, the -1
    dropped, the stored value two steps of the format off, the fp32 polynomial's switch at -5.  NOT caught, by construction:
    truncation instead of round-to-nearest-even at the store after the ELU: a truncated value is less than one step from the
    rounded one, and one step is what the bound grants the two half-step roundings (the bit-exact fixtures pin the store's
    rounding on the same kernels' identity side).  The worst truncation ratio is asserted to lie in (1/2, 1]: the bound is
    within a factor two of the smallest that a correct kernel needs."""
    z = _operands(fx, SHAPES[0], dtype)
    e = np.expm1(z)
    r = ec.ROUND[dtype]
    want = r(torch.from_numpy(e)).numpy()
    bound = ec.step16(dtype, e) + ec.ELU_16_ABS

    def ratio(v32, store=r):
        return float((np.abs(store(torch.from_numpy(np.asarray(v32, np.float64))).numpy() - want) / bound).max())
    f = ec.elu_cancelling_form(z)
    assert ratio(f) <= 1
    ex = np.exp(z.astype(np.float32).astype(np.float64)).astype(np.float32)
    assert ratio(ex + np.float32(1)) > 1 and ratio(ex) > 1
    assert ratio(ec.elu_f32_form(z, switch=-5.0)) > 1
    stored = r(torch.from_numpy(f.astype(np.float64))).numpy()
    assert ratio(stored - 2 * ec.step16(dtype, stored), store=lambda t: t) > 1
    t = ratio(f, store=ec.TRUNCATE[dtype])
    print("\n%s %s: truncating store, worst error / bound %.3f" % (fx["name"], dtype, t))
    assert 0.5 < t <= 1


# ------------------------------------------------------------------------------------------------------------ fp16 subnormals
def _flush_f16(t):
    """fp16 rounding that flushes subnormal results to zero (the fault the f16sub fixtures must bite on)."""
    r = ec._r_f16(t)
    return torch.where(r.abs() < 2.0 ** -14, torch.zeros_like(r), r)


def _first_small(fx):
    """reference() name of the first tensor of an f16sub fixture that holds subnormals."""
    c = fx["f16sub"]["down"][0].split(".")
    return "model.%s.dw" % c[1] if c[0] == "model" and c[1] != "0" and c[2] == "0" else fx["layers"][0]


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("fx", ec.F16SUB_FIXTURES, ids=[f["name"] for f in ec.F16SUB_FIXTURES])
def test_f16sub_fixtures_store_and_consume_the_named_subnormals(fx, shape):
    """At fp16 the first scaled tensor holds 2^-14, the largest subnormal, 2^-24, exact ties of the subnormal grid that round to
    even upwards and downwards, and non-zero values that round to 0; it is torch's half rounding of the fp32 fixture's tensor
    (so the values in front of it are the same at both dtypes); every tensor up to the consumer holds subnormals; the consumer's
    output is normal again and changes when subnormals are flushed to zero at any rounding point."""
    t = 2.0 ** -24
    r32, r16 = ec.fixture_reference(fx, shape, "fp32"), ec.fixture_reference(fx, shape, "fp16", probe=True)
    name = _first_small(fx)
    pre, post = r32[name], r16[name]
    assert np.array_equal(post, ec._r_f16(torch.from_numpy(pre)).numpy())
    u, v = pre / t, post / t
    tie = u % 1 == 0.5
    assert (post == 2.0 ** -14).any() and (post == 1023 * t).any() and (post == t).any(), fx["name"]
    assert (tie & (v > u)).any() and (tie & (v < u) & (v > 0)).any() and ((pre != 0) & (post == 0)).any(), fx["name"]
    st = r16["_stored"]
    last = ec.last_layer(fx)
    for layer in fx["layers"][:-1]:
        key = layer + ".cat" if layer.endswith(".heads.1") else layer
        assert st[key][0] < 2.0 ** -14, (fx["name"], layer)          # subnormals stored (or handed to the MFMA) all the way
    assert st[last][0] >= 2.0 ** -14 and fx["f16sub"]["up"] in fx["convs"][-1:]
    flushed = ec.reference(ec.dense_sd(fx), ec.frame_of(shape), fx["nref"], "fp16", round16=_flush_f16, stop_after=last)
    assert not np.array_equal(flushed[last], r16[last]), fx["name"]
    assert not np.array_equal(flushed[name], post), fx["name"]
    trunc = ec.fixture_reference(fx, shape, "fp16", rounding="truncate")
    assert not np.array_equal(trunc[last], r16[last]) and not np.array_equal(trunc[name], post), fx["name"]


def test_f16sub_fixtures_take_every_route_and_every_layer_kind_of_the_bf16_rows():
    """Routes: a depthwise unpack, an MFMA activation operand, the residual and the concat copy, a subnormal packed GEMM weight.
    Closure: every bf16 row of tests/variant_matrix.py (stem, the three fused depthwise + pointwise forms, 1x1 and 3x3 GEMM,
    window-resident 3x3 with and without the folded 1x1, heads) lists a layer that some f16sub fixture has under test, so
    tests/test_gpu_exact.py forces that kernel on subnormals at fp16."""
    import variant_matrix as vm
    specs = {f["name"]: f["f16sub"] for f in ec.F16SUB_FIXTURES}
    ups = {s["up"] for s in specs.values()}
    assert {"model.1.0", "model.2.0", "model.5.0", "model.7.0"} <= ups                               # depthwise unpack (stride 2, dilation 2)
    assert {"model.5.3", "cpm.conv.0", "refinement_stages.0.trunk.0.initial.0", "refinement_stages.0.trunk.1.initial.0"} <= ups   # MFMA operand
    assert "cpm.trunk.2.2" in specs["f16sub:cpm"]["mid"] and "refinement_stages.0.trunk.0.trunk.1.0" in specs["f16sub:refinement"]["mid"]   # residual
    assert "initial_stage.pafs.1.0" in specs["f16sub:cpm.conv>concat"]["mid"]                        # concat copy of the stage maps
    packed = [c for s in specs.values() for c in s["down"] if not c.startswith("model.") or c.endswith(".3")]
    assert len(packed) >= 6 and ec.F16SUB_DOWN < 2.0 ** -14 and ec.F16SUB_DOWN / 2.0 ** -24 == 128   # 2^-17: a subnormal fp16 weight
    under = {l for f in ec.F16SUB_FIXTURES for l in f["layers"]}
    rows = [r for r in vm.ROWS if r["dtype"] == "bf16"]
    assert len(rows) >= 48 and {r["family"] for r in rows} == {"stem", "dwpw_bf16", "dwpw_tiled", "dwpw_bf16_pp", "heads_bf16", "gemm_bf16", "gemm_bf16_ar"}
    missing = [(r["variant"], r["layers"]) for r in rows if not under & set(r["layers"])]
    assert not missing, missing
    kinds = {r["variant"] for r in rows if under & set(r["layers"])}
    assert any(v.endswith("+1x1") for v in kinds) and any(v.startswith("gemm_bf16_ar<") and not v.endswith("+1x1") for v in kinds)


# ------------------------------------------------------------------------------------------------------------ fp16 overflow
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
@pytest.mark.parametrize("fx", ec.F16OVF_FIXTURES, ids=[f["name"] for f in ec.F16OVF_FIXTURES])
def test_f16ovf_fixtures_store_the_named_values_and_one_consumer_reads_them(fx, shape):
    """The scaled tensor holds 65504, values in (65504, 65520), the tie 65520 and larger values, all finite in f32 (the heads
    fixture: each with its negative twin, in the f32 stage outputs, while the 16-bit concat copy is +-inf); at fp16 it is
    torch's half rounding of that: 65504 stays, the open interval rounds to 65504, 65520 and above to inf.  The consumer holds
    NaN (inf x 0), inf and ordinary numbers; saturating at 65504 instead of rounding to inf changes both tensors; at fp32
    and bf16 everything is finite."""
    spec = fx["f16ovf"]
    r32, r16 = ec.fixture_reference(fx, shape, "fp32"), ec.fixture_reference(fx, shape, "fp16")
    name = ec._first_tensor(spec)
    heads = name.endswith(".heads.1")
    pre, post = (r16[name], r16[name + ".cat"]) if heads else (r32[name], r16[name])
    assert np.isfinite(pre).all() and np.array_equal(post, ec._r_f16(torch.from_numpy(pre)).numpy())
    for sg in (1, -1) if spec.get("twins") else (1,):
        v, r = sg * pre, sg * post
        assert (v == 65504).any() and ((v > 65504) & (v < 65520)).any() and (v == 65520).any() and (v > 65520).any(), (fx["name"], sg)
        assert np.all(r[(v >= 65504) & (v < 65520)] == 65504) and np.all(np.isposinf(r[v >= 65520])), (fx["name"], sg)
    last = ec.last_layer(fx)
    out = r16[last]
    assert np.isnan(out).any() and (np.isfinite(out) & (out != 0)).sum() >= 1000, fx["name"]
    for dtype in ("fp32", "bf16"):
        assert all(np.isfinite(v).all() for k, v in ec.fixture_reference(fx, shape, dtype).items() if not k.startswith("_")), (fx["name"], dtype)

    def saturate(t):
        return torch.clamp(ec._r_f16(t), -65504.0, 65504.0)
    sat = ec.reference(ec.dense_sd(fx), ec.frame_of(shape), fx["nref"], "fp16", round16=saturate, stop_after=last)
    key = name + ".cat" if heads else name
    assert np.isfinite(sat[key]).all() and np.isfinite(sat[last]).all()
    assert not np.array_equal(sat[key], post) and not np.array_equal(np.isnan(sat[last]), np.isnan(out)), fx["name"]


def test_f16ovf_fixtures_cover_every_layer_kind_of_the_bf16_rows():
    """As for f16sub: every bf16 row of the variant matrix lists a layer that some f16ovf fixture has under test, as the layer
    that stores the overflow or as the one consumer that reads it; the heads fixture carries the negative twins."""
    import variant_matrix as vm
    assert len(ec.F16OVF_FIXTURES) == 11 and sum(1 for f in ec.F16OVF_FIXTURES if f["f16ovf"].get("twins")) == 1
    assert all(len(f["layers"]) <= 2 for f in ec.F16OVF_FIXTURES)                # one consumer
    under = {l for f in ec.F16OVF_FIXTURES for l in f["layers"]}
    rows = [r for r in vm.ROWS if r["dtype"] == "bf16"]
    missing = [(r["variant"], r["layers"]) for r in rows if not under & set(r["layers"])]
    assert len(rows) >= 48 and not missing, missing
    kinds = {r["variant"] for r in rows if under & set(r["layers"])}
    assert any(v.endswith("+1x1") for v in kinds) and any(v.startswith("gemm_bf16_ar<") and not v.endswith("+1x1") for v in kinds)
    assert {r["family"] for r in rows} == {"stem", "dwpw_bf16", "dwpw_tiled", "dwpw_bf16_pp", "heads_bf16", "gemm_bf16", "gemm_bf16_ar"}
