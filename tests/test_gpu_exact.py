"""Every conv kernel bit for bit against float64 on the exact-arithmetic fixtures of tests/exact_cases.py (-m gpu).

On those fixtures every product and partial sum is exactly representable in fp32 (tests/test_exact_host.py checks it on the
CPU), so whatever kernel, tile, split-K or fusion runs a layer, its output is one known number per element, rounded once to
nearest even where the path stores 16 bits.  ``np.array_equal`` on every element; there is no tolerance and nothing is left out.

  * default kernels: every fixture x {fp32, bf16, fp16} x {2, 1} frames; a fused group is read at its last layer and at every
    member ``debug_layer_output`` exposes; stage outputs are read twice, as the f32 maps ``forward`` returns and as their
    (16-bit) copy in the concat buffer;
  * every row of tests/variant_matrix.py, forced with the row's switches (bf16 rows also at fp16): the row's variant string is
    asserted and each of its layers runs every fixture that has it under test, the joint ones of its fused group included.
    Not run: dw<px=2>, which only a 720 x 1280 frame reaches (a workload-size frame).

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
SKIPPED_VARIANT = "dw<px=2>"             # no switch: pixels * C / 4 >= 2^20, a 720 x 1280 frame

REPORT = {"cases": [], "variants_seen": {}}


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


_CASES = [(dtype, shape, fx) for dtype in ec.DTYPES for shape in ec.FRAMES for fx in ec.FIXTURES]


@pytest.mark.parametrize("dtype,shape,fx", _CASES, ids=["%s-b%d-%s" % (d, s[0], f["name"]) for d, s, f in _CASES])
def test_default_kernels_bit_for_bit(monkeypatch, dtype, shape, fx):
    eng = default_engine(monkeypatch, dtype, fx["nref"])
    bad = []
    check("default-%s-b%d-%s" % (dtype, shape[0], fx["name"]), eng, fx, shape, dtype, _layers_in(eng, fx), bad)
    assert not bad, bad


def _row_id(r, dtype):
    env = ",".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items()))
    return "%s-%s-%s-%s" % (dtype, r["variant"], env or "default", r["layers"][0])


_ROWS = [(r, dt) for r in vm.ROWS if r["variant"] != SKIPPED_VARIANT for dt in ([r["dtype"]] + (["fp16"] if r["dtype"] == "bf16" else []))]


def test_only_the_workload_size_depthwise_row_is_left_out():
    left = [r for r in vm.ROWS if r["variant"] == SKIPPED_VARIANT]
    assert len(left) == 1 and left[0]["frame"] == (1, 720, 1280)
    assert all(r["frame"] == vm.FRAME for r, _ in _ROWS) and vm.FRAME == ec.FRAMES[0]


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
