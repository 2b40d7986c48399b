"""CPU (-m "not gpu"): the 16-bit mode of the backward (lwp_set_backward_precision) as far as it can be checked without a GPU: the
exports, the argument rules that need no device, the statements of tests/backward_h16_cases.py on the integer fixtures (where no
operand rounds, so they must equal the f32 statements exactly), mutants of those statements against the normal fixtures (a
fixture on which a wrong rounding, a missing 1 / grad_scale or a rounded bias sum goes unseen has no teeth), and the end-to-end
restatement: with no rounding it is the plain float64 restatement, and the error the formats cost (e_sim) lies strictly between
the fp32 reference error e_ref and 0.1 on the cases tests/test_gpu_backward_h16.py runs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from oracle import net_ref

import backbone_backward_cases as bb
import backward_cases as bc
import backward_h16_cases as hc
import backward_kernel_cases as kc
import exact_cases as ec
import train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda shapes: ["x".join(str(v) for v in s) for s in shapes]


# ---------------------------------------------------------------------------------------------- exports and argument rules
def test_exports_are_declared_and_present_and_the_version_moved():
    header = open(os.path.join(ROOT, "include", "lwpose.h")).read()
    L = _lib.lib()
    for name in ("lwp_set_backward_precision", "lwp_get_backward_precision"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert "int %s(lwp_handle h, " % name in header
    assert L.lwp_version() >= 107
    assert _lib.BACKWARD_PRECISIONS == {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}
    for words in ("no 16-bit backward", "a 16-bit backward"):
        for path in ("README.md", "include/lwpose.h", "lightweight-human-pose-estimation.pytorch_amd/optim.py"):
            assert words not in open(os.path.join(ROOT, path)).read(), (words, path)


def test_a_null_handle_is_refused_without_a_gpu():
    L = _lib.lib()
    dt, sc = C.c_int(), C.c_double()
    assert L.lwp_set_backward_precision(None, _lib.BF16, 1.0) == _lib.LWP_ERR_ARG
    assert L.lwp_get_backward_precision(None, C.byref(dt), C.byref(sc)) == _lib.LWP_ERR_ARG
    assert L.lwp_last_error(None)


# ---------------------------------------------------------------------------------------------- the statements
def flags_of(shape):
    return [(a, nb, acc) for a in kc.acc_from_values(shape[4]) for nb in (0, 1) for acc in (0, 1)]


def test_shapes_cross_the_k_step_they_name():
    s33, s31, s64 = hc.K_STEP_SHAPES
    assert kc.dense_M(s33) == 33 and s33[3] == 33
    assert kc.dense_M(s31) == 31 and s31[3] == 31 and s31[5] == 3
    assert kc.dense_M(s64) == 32 and s64[3] == 64 and s64[7] == "raw" and s64[3] % 16 == 0 and s64[4] % 4 == 0
    assert hc.DENSE_SHAPES[:len(kc.DENSE_SHAPES)] == kc.DENSE_SHAPES and hc.CHUNKS == (0, 16, 48)
    assert all(c % 16 == 0 for c in hc.CHUNKS)
    for shape in hc.DENSE_SHAPES:
        cout_pad, cin_pad = kc.dense_pads(shape)
        assert shape[3] <= cout_pad and shape[4] <= cin_pad and cin_pad % 4 == 0 and cout_pad % 16 == 0


@pytest.mark.parametrize("shape", hc.DENSE_SHAPES, ids=ids(hc.DENSE_SHAPES))
def test_integer_fixtures_are_exact_in_both_formats_and_equal_the_f32_statement(shape):
    f = kc.dense_fixture(shape, "int")
    for k, v in f.items():
        assert v.dtype == np.int64 and np.abs(v).max() <= (64 if k.endswith("0") else 8), k
    for precision, S in hc.MODES:
        # operands: |dz| S <= 512 and |x|, |w| <= 8 are integers of at most 10 bits, exact in bf16 (8) only below 256: scale 1 there
        assert np.array_equal(hc.round16(f["dz"] * S, precision), f["dz"] * S) and np.array_equal(hc.round16(f["x"], precision), f["x"])
        assert np.array_equal(hc.round16(f["w"], precision), f["w"])
        # scaled products and partial sums stay below 2^24 (prior contents are added after the 1 / S)
        _, terms = kc.dense_results(f["dz"] * int(S), f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], 0, 0, 1)
        assert kc.max_terms(terms) < kc.EXACT_LIMIT
        for a, nb, acc in flags_of(shape):
            want, _ = kc.dense_results(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, nb, acc)
            got, _ = hc.dense_results_h16(f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], a, nb, acc, precision, S)
            for k in want:
                assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), (shape, precision, S, a, nb, acc, k)


@pytest.mark.parametrize("precision,S", hc.MODES)
def test_mutants_of_the_statement_differ_on_the_normal_fixtures(precision, S):
    """Truncation instead of rounding, a missing 1 / grad_scale (visible at S != 1 only) and a bias sum over the rounded dz."""
    seen = dict(truncate=0, unscaled=0, round_db=0)
    for shape in hc.DENSE_SHAPES:
        f = kc.dense_fixture(shape, "normal")
        args = (f["dz"], f["x"], f["w"], shape[6], f["dx0"], f["dw0"], f["db0"], shape[4], 0, 0, precision, S)
        true, terms = hc.dense_results_h16(*args)
        depths = kc.dense_depths(shape, shape[4], 0)
        mutants = dict(truncate=hc.dense_results_h16(*args, rounding=ec.TRUNCATE)[0], unscaled=hc.dense_results_h16(*args, unscale=False)[0],
                       round_db=hc.dense_results_h16(*args, round_db=True)[0])
        assert all(v <= 1.0 for v in hc.bound_ratios_h16(true, true, terms, depths).values())
        for name, m in mutants.items():
            r = hc.bound_ratios_h16(m, true, terms, depths)
            seen[name] += any(not v <= 1.0 for v in r.values())       # the GPU test's comparison reports it
    assert seen["truncate"] == len(hc.DENSE_SHAPES) and seen["round_db"] >= 1
    assert seen["unscaled"] == (len(hc.DENSE_SHAPES) if S != 1 else 0)


def test_the_statement_rounds_to_nearest_even_keeps_subnormals_and_overflows_to_infinity():
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 2.0 ** -24, 65520.0, 1e39])
    assert np.array_equal(hc.round16(v, "bf16"), [1.0, 1.0 + 2.0 ** -6, 2.0 ** -24, 65536.0, np.inf])           # ties to even; float32's range
    w = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -24, 2.0 ** -26, 65519.0, 65520.0])
    assert np.array_equal(hc.round16(w, "fp16"), [1.0, 1.0 + 2.0 ** -9, 2.0 ** -24, 0.0, 65504.0, np.inf])
    assert hc.fp16_scale(1.0) == 2.0 ** 14 and hc.fp16_scale(0.99) == 2.0 ** 15 and hc.fp16_scale(1e-30) == 2.0 ** 24 and hc.fp16_scale(1e6) == 1.0


# ---------------------------------------------------------------------------------------------- end to end
def e2e_inputs(scope):
    """(case, args of GRADIENTS[scope]) on the CPU: the restatement starts at the float64 oracle's activation (the GPU test starts
    at the device's own), targets from the NumPy restatement."""
    cases, name = hc.E2E_CASES[scope]
    c = cases[name]
    NH, NP = bc.channels(c)
    sd = synth.make_state_dict(c["nref"], seed=c["seed"], num_channels=c["C"], num_heatmaps=NH, num_pafs=NP)
    fr = synth.make_frames(c["N"], c["H"], c["W"], seed0=c["frames"])
    x = np.ascontiguousarray(((fr.astype(np.float32) - 128.0) * np.float32(1 / 256)).transpose(0, 3, 1, 2))
    K, lk, lp = tc.skeleton(c["skel"])
    kp, n = bc.persons(c)
    hs, ws = bb.map_dims(c)
    km, pm = tc.targets(kp, n, 8 * hs, 8 * ws, 8, 7, 1, K, tc.limb_rows(lk, lp))
    mask = bb.loss_mask(c) if scope == "all" else bc.loss_mask(c)
    if scope == "all":
        start = torch.from_numpy(x)
    else:
        taps = {}
        net_ref.forward64(sd, torch.from_numpy(x), c["nref"], taps, stop_after="cpm")
        start = (taps["cpm"] if scope == "stages" else taps["model.11"]).to(torch.float32)      # the device hands over float32
    return c, (sd, start, c["nref"], torch.from_numpy(km), torch.from_numpy(pm), torch.from_numpy(mask), c["N"])


def test_the_smallest_case_of_each_scope():
    assert dict((s, n) for s, (_, n) in hc.E2E_CASES.items()) == dict(stages="d", cpm="f", all="t")


@pytest.mark.parametrize("scope", ["stages", "cpm", "all"])
def test_e_sim_lies_between_the_fp32_reference_error_and_a_tenth(scope):
    c, args = e2e_inputs(scope)
    grad = hc.GRADIENTS[scope]
    g32, taps32 = grad(*args, dtype=torch.float32)[:2]
    masks = bc.own_masks(taps32)
    g64 = grad(*args, masks=masks)[0]
    e_ref = max(bc.err(g32[k], g64[k]) for k in g64)
    # without rounding the replaced backward is the plain one (another summation order inside torch at the most)
    plain, stats = hc.sim_gradients(scope, "fp32", 1.0, *args, masks=masks)
    assert set(plain) == set(g64) and stats["nonzero"] > 0 and stats["flushed"] == 0
    for k in g64:
        assert bc.err(plain[k], g64[k]) <= 1e-12, k
    for precision in ("bf16", "fp16"):
        S = 1.0 if precision == "bf16" else hc.fp16_scale(stats["max_dz"])
        if precision == "fp16":
            assert 1.0 <= S <= 2.0 ** 24 and stats["max_dz"] * S < 2.0 ** 15 and (S == 2.0 ** 24 or stats["max_dz"] * 2 * S >= 2.0 ** 15)
        sim, st = hc.sim_gradients(scope, precision, S, *args, masks=masks)
        assert all(torch.isfinite(v).all() for v in sim.values())
        e_sim = max(bc.err(sim[k], g64[k]) for k in g64)
        print("scope %s case %s %s scale %g: e_sim %.3g, e_ref %.3g, %d of %d non-zero dz flushed" %
              (scope, hc.E2E_CASES[scope][1], precision, S, e_sim, e_ref, st["flushed"], st["nonzero"]))
        assert e_ref < e_sim < 0.1, (scope, precision, e_sim, e_ref)
