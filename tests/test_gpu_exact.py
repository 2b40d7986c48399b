"""Every conv kernel bit for bit against float64 on the exact-arithmetic fixtures of tests/exact_cases.py (-m gpu).

On those fixtures every product and partial sum is exactly representable in fp32 (tests/test_exact_host.py checks it on the
CPU), so whatever kernel, tile, split-K or fusion runs a layer, its output is one known number per element, rounded once to
nearest even where the path stores 16 bits.  ``np.array_equal`` on every element; there is no tolerance and nothing is left out.

  * default kernels: every fixture x {fp32, bf16, fp16} x {2, 1} frames; a fused group is read at its last layer and at every
    member ``debug_layer_output`` exposes; stage outputs are read twice, as the f32 maps ``forward`` returns and as their
    (16-bit) copy in the concat buffer;
  * every row of tests/variant_matrix.py at the fixture frame, forced with the row's switches (bf16 rows also at fp16): the
    row's variant string is asserted and each of its layers runs every fixture that has it under test, the joint ones of its
    fused group included.  dw<px=2> runs here too (LWP_DW_PX=2, odd output widths); no variant of the matrix is left out.

The ``f16sub:*`` fixtures are among them: at fp16 they store and consume subnormals (2^-14, the largest subnormal, 2^-24, ties
of the subnormal grid, non-zero values that round to 0) in every kernel family; the oracle is torch's CPU half rounding, so a
flush at a store or at an MFMA / depthwise operand differs.  The ``f16ovf:*`` fixtures store 65504, values that round to it,
the tie 65520 and larger values (fp16: inf, never saturated) and read one consumer; for them alone a NaN (inf x 0) at the same
place as in the reference counts as equal, and inf equals inf of the same sign as always.

ELU below zero is pinned by a bound, not bit for bit (the ``elu:*`` fixtures of tests/exact_cases.py, which states the bounds
and their derivation): per element behind an exactly known negative operand, fp32 within 1e-6 relative of float64 expm1, bf16
and fp16 within one step of the format + 2^-22 of the rounded expm1; the result lies in [-1, 0]; z = 0 gives 0 and the positive
elements of the same tensors are bit exact.  Default engines (three dtypes x both frames) and every row that lists a
cpm.trunk layer; behind a forced stand-alone depthwise the f32 GEMM's ELU epilogue is read as well.  The worst error / bound
per dtype and variant is printed and lands in the report under "elu_worst".

LWP_EXACT_REPORT=path dumps per comparison the variant seen, the elements compared and the elements differing."""
import json
import os

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine

import exact_cases as ec
import variant_matrix as vm

pytestmark = pytest.mark.gpu

DT = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}
# every kernel-choice switch a row may set: cleared before each engine so that one row's switch never leaks into another's
SWITCHES = sorted({k for r in vm.ROWS for k in r["env"]} | {k for u in vm.UPSAMPLE_ROWS for k in u["env"]} | {"LWP_MS_TX"})

REPORT = {"cases": [], "variants_seen": {}, "elu": [], "elu_worst": {}}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("LWP_EXACT_REPORT")
    if path:
        REPORT["totals"] = dict(comparisons=len(REPORT["cases"]), compared=sum(c["compared"] for c in REPORT["cases"]),
                                differing=sum(c["differing"] for c in REPORT["cases"]))
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


def make_engine(monkeypatch, env, dtype, nref=1):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(0, nref=nref, dtype=DT[dtype])
    eng.load_state_dict(ec.selector(nref))
    for k in env:
        monkeypatch.delenv(k)
    return eng


_DEFAULT, _REF = {}, {}


def default_engine(monkeypatch, dtype, nref):
    if (dtype, nref) not in _DEFAULT:
        _DEFAULT[(dtype, nref)] = make_engine(monkeypatch, {}, dtype, nref)
    return _DEFAULT[(dtype, nref)]


def reference(fx, shape, dtype):
    key = (fx["name"], shape, dtype)
    if key not in _REF:
        _REF[key] = ec.fixture_reference(fx, shape, dtype)
    return _REF[key]


def f16_twin(variant):
    return "stem_f16<" + variant[len("stem<"):] if variant.startswith("stem<") else variant.replace("bf16", "f16")


def check(case, eng, fx, shape, dtype, layers, bad, expect_variant=None):
    """Load the fixture and compare each of ``layers`` (and the f32 stage outputs behind a ``.heads.1``) with the reference."""
    x = ec.frame_of(shape)
    ref = reference(fx, shape, dtype)
    idx = {l["name"]: l["index"] for l in eng.layers()}
    eng.load_state_dict(ec.dense_sd(fx))

    def note(layer, variant, got, want):
        assert got.shape == want.shape, (fx["name"], layer, got.shape, want.shape)
        differ = got.astype(np.float64) != want                   # as numbers: -0 == 0; a NaN differs
        if fx.get("nonfinite_ok"):                                # the f16ovf fixtures only: NaN at the same place is equal (inf of
            differ &= ~(np.isnan(got) & np.isnan(want))           # the same sign already is: inf == inf, inf != -inf)
        n = int(differ.sum())
        REPORT["cases"].append(dict(case=case, dtype=dtype, frame=list(shape), fixture=fx["name"], layer=layer, variant=variant,
                                    compared=int(want.size), differing=n))
        if n:
            at = tuple(int(v) for v in np.argwhere(differ)[0])
            bad.append((fx["name"], layer, variant, "%d of %d differ" % (n, want.size), at, float(got[at]), float(want[at])))
        elif variant is not None:
            seen = REPORT["variants_seen"].setdefault(variant, [])
            if layer not in seen:
                seen.append(layer)

    for layer in sorted(layers, key=lambda n: idx[n]):
        got = eng.debug_layer_output(x, idx[layer])
        variant = eng.layer_variant(idx[layer])
        if expect_variant is not None and variant != expect_variant:
            bad.append((fx["name"], layer, "variant", variant, expect_variant))
        stage_copy = layer.endswith(".heads.1") and dtype != "fp32"
        note(layer, variant, got, ref[layer + ".cat" if stage_copy else layer])
        if layer.endswith(".heads.1"):                              # the f32 stage outputs of the same kernels
            stage = layer[:-len(".heads.1")]
            k = 0 if stage == "initial_stage" else 1 + int(stage.split(".")[1])
            outs = eng.forward(x)
            note(layer + " (f32 outputs)", variant, np.concatenate([outs[2 * k], outs[2 * k + 1]], axis=1), ref[layer])


def _layers_in(eng, fx):
    have = {l["name"] for l in eng.layers()}
    out = []
    for layer in fx["layers"]:
        if layer.endswith(".pw") and layer[:-3] + ".dw" in have:
            out.append(layer[:-3] + ".dw")                          # the unfused graph exposes the depthwise result too
        assert layer in have, layer
        out.append(layer)
    return out


_CASES = [(dtype, shape, fx) for dtype in ec.DTYPES for shape in ec.FRAMES for fx in ec.ALL_EXACT]


@pytest.mark.parametrize("dtype,shape,fx", _CASES, ids=["%s-b%d-%s" % (d, s[0], f["name"]) for d, s, f in _CASES])
def test_default_kernels_bit_for_bit(monkeypatch, dtype, shape, fx):
    eng = default_engine(monkeypatch, dtype, fx["nref"])
    bad = []
    check("default-%s-b%d-%s" % (dtype, shape[0], fx["name"]), eng, fx, shape, dtype, _layers_in(eng, fx), bad)
    assert not bad, bad


def _row_id(r, dtype):
    env = ",".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items()))
    return "%s-%s-%s-%s" % (dtype, r["variant"], env or "default", r["layers"][0])


_ROWS = [(r, dt) for r in vm.ROWS if r["frame"] == vm.FRAME for dt in ([r["dtype"]] + (["fp16"] if r["dtype"] == "bf16" else []))]


def test_no_variant_of_the_matrix_is_left_out():
    """Every (variant, dtype) of the matrix runs here at the fixture frame; the only row at another size (the 720 x 1280 frame
    at which the heuristic itself takes dw<px=2>: tests/test_kernel_variants.py) repeats a variant that a forced row has."""
    assert vm.FRAME == ec.FRAMES[0]
    ran = {(r["variant"], r["dtype"]) for r, _ in _ROWS}
    assert ran == {(r["variant"], r["dtype"]) for r in vm.ROWS} and ("dw<px=2>", "fp32") in ran
    other = [r for r in vm.ROWS if r["frame"] != vm.FRAME]
    assert [(r["variant"], r["frame"]) for r in other] == [("dw<px=2>", (1, 720, 1280))]
    assert {dt for r, dt in _ROWS if r["dtype"] == "bf16"} == {"bf16", "fp16"}


@pytest.mark.parametrize("row,dtype", _ROWS, ids=[_row_id(r, dt) for r, dt in _ROWS])
def test_forced_variant_bit_for_bit(monkeypatch, row, dtype):
    eng = make_engine(monkeypatch, row["env"], dtype)
    want = f16_twin(row["variant"]) if dtype == "fp16" else row["variant"]
    bad, ran = [], 0
    for layer in row["layers"]:
        fixtures = ec.fixtures_for(layer)
        assert fixtures, layer
        for fx in fixtures:
            check(_row_id(row, dtype), eng, fx, row["frame"], dtype, [layer], bad, expect_variant=want)
            ran += 1
    assert ran >= len(row["layers"]) and not bad, bad


# ------------------------------------------------------------------------------------------------------------ ELU below zero
_ELU_REF = {}


def elu_reference(fx, shape, dtype):
    key = (fx["name"], shape, dtype)
    if key not in _ELU_REF:
        _ELU_REF[key] = ec.elu_reference(fx, shape, dtype)
    return _ELU_REF[key]


def check_elu(case, eng, fx, shape, dtype, layers, bad, expect=None):
    """Load the ELU fixture and hold each of ``layers`` to ``ec.elu_expect``; ``expect`` = {layer: variant it must record}."""
    x = ec.frame_of(shape)
    ref = elu_reference(fx, shape, dtype)
    idx = {l["name"]: l["index"] for l in eng.layers()}
    eng.load_state_dict(ec.dense_sd(fx))
    for layer in sorted(layers, key=lambda n: idx[n]):
        got = eng.debug_layer_output(x, idx[layer])
        variant = eng.layer_variant(idx[layer])
        if expect and layer in expect and variant != expect[layer]:
            bad.append((fx["name"], layer, "variant", variant, expect[layer]))
        exp = ec.elu_expect(fx, ref, layer, dtype)
        assert got.shape == exp["want"].shape, (fx["name"], layer, got.shape)
        problems, ratio = ec.elu_compare(got, exp)
        print("%s %s b%d %s %s [%s]: worst error / bound %.4f over %d negative operands" % (
            case, dtype, shape[0], fx["name"], layer, variant, ratio, int(exp["neg"].sum())))
        REPORT["elu"].append(dict(case=case, dtype=dtype, frame=list(shape), fixture=fx["name"], layer=layer, variant=variant,
                                  negative_operands=int(exp["neg"].sum()), exact_elements=int((~exp["neg"]).sum()),
                                  worst_error_over_bound=ratio, problems=problems))
        worst = REPORT["elu_worst"].setdefault(dtype, {})
        worst[str(variant)] = max(worst.get(str(variant), 0.0), ratio)
        bad += [(fx["name"], layer, variant, p) for p in problems]


_ELU_CASES = [(dtype, shape, fx) for dtype in ec.DTYPES for shape in ec.FRAMES for fx in ec.ELU_FIXTURES]


@pytest.mark.parametrize("dtype,shape,fx", _ELU_CASES, ids=["%s-b%d-%s" % (d, s[0], f["name"]) for d, s, f in _ELU_CASES])
def test_default_kernels_elu_below_zero(monkeypatch, dtype, shape, fx):
    eng = default_engine(monkeypatch, dtype, fx["nref"])
    bad = []
    check_elu("default", eng, fx, shape, dtype, _layers_in(eng, fx), bad)
    assert not bad, bad


_ELU_ROWS = [(r, dt) for r, dt in _ROWS if any(l.startswith("cpm.trunk.") for l in r["layers"])]


def test_elu_rows_cover_every_kernel_family_that_runs_the_cpm_trunk():
    fam = {(r["family"], dt) for r, dt in _ELU_ROWS}
    assert fam == {("dw", "fp32"), ("dw_tiled", "fp32"), ("dwpw", "fp32"), ("dwpw_bf16", "bf16"), ("dwpw_bf16", "fp16"),
                   ("dwpw_tiled", "bf16"), ("dwpw_tiled", "fp16")}, fam
    assert {r["variant"] for r, _ in _ELU_ROWS if r["family"] == "dw"} == {"dw<px=1>", "dw<px=2>"}


@pytest.mark.parametrize("row,dtype", _ELU_ROWS, ids=[_row_id(r, dt) for r, dt in _ELU_ROWS])
def test_forced_variant_elu_below_zero(monkeypatch, row, dtype):
    eng = make_engine(monkeypatch, row["env"], dtype)
    want = f16_twin(row["variant"]) if dtype == "fp16" else row["variant"]
    bad, ran = [], 0
    for layer in row["layers"]:
        if not layer.startswith("cpm.trunk."):
            continue
        fixtures = ec.elu_fixtures_for(layer)
        assert len(fixtures) == 2, layer
        # behind a stand-alone depthwise the pointwise conv is a GEMM with an ELU epilogue of its own: read it as well
        layers = [layer, layer[:-3] + ".pw"] if layer.endswith(".dw") else [layer]
        for fx in fixtures:
            check_elu(_row_id(row, dtype), eng, fx, row["frame"], dtype, layers, bad, expect={layer: want})
            ran += 1
    assert ran and not bad, bad
