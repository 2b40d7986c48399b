"""LWP_F16 (IEEE half storage / fp16 MFMA, f32 accumulation) on the GPU (-m gpu), through the C-ABI.

Bars fixed from the CPU emulation (tools/f16_budget.py: stage outputs max-abs 0.003-0.0065 x scale, mean-abs 0.0008 x scale,
99 % of key-points matched) with about 3x margin: F16_TOL / F16_MEAN x scale, scale = max(1, max|reference|).  A miss while
the emulation meets them points at a kernel (rounding mode, denormal flush, fragment layout), not at the bar."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth, workload
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine
from oracle import net_ref, post_ref

import variant_matrix as vm
from conftest import ROOT

pytestmark = pytest.mark.gpu

F16_TOL = 0.02
F16_MEAN = 0.0025
# another kernel on the same input: one fp16 rounding step (2^-10 relative) plus a small absolute term (scale-relative)
F16_STEP = 2.0 ** -10
F16_ABS = 1e-4


def net_input(n, h, w, seed):
    fr = synth.make_frames(n, h, w, seed0=seed)
    x = (fr.astype(np.float32) - 128.0) * np.float32(1 / 256)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _f16_net(nref=1, seed=1):
    net = PoseEstimationWithMobileNet(num_refinement_stages=nref, dtype="fp16")
    sd = synth.make_state_dict(nref, seed=seed)
    load_state(net, {"state_dict": sd})
    return net.eval().cuda(), sd


_CAL = {}


def _calibrated():
    if "net" not in _CAL:
        _CAL["net"] = workload.build_net(nref=1, seed=1, device=0, dtype="fp16")
    return _CAL["net"]


def _within(got, ref, what):
    sc = max(1.0, float(np.abs(ref).max()))
    d = np.abs(got.astype(np.float64) - ref)
    assert d.max() <= F16_TOL * sc and d.mean() <= F16_MEAN * sc, (what, float(d.max()) / sc, float(d.mean()) / sc)


def _f16_twin(variant):
    return "stem_f16<" + variant[len("stem<"):] if variant.startswith("stem<") else variant.replace("bf16", "f16")


@pytest.mark.parametrize("nref", [1, 3])
def test_f16_per_layer_and_outputs_within_tolerance(nref):
    net, sd = _f16_net(nref)
    x = net_input(2, 67, 101, seed=100)                  # ragged: 34 x 51 / 17 x 26 / 9 x 13 maps
    taps = {}
    outs = net_ref.forward(sd, torch.from_numpy(x), nref, taps)
    eng = net.engine
    checked = 0
    for info in eng.layers():
        nm = info["name"]
        key = nm[:-3] if nm.endswith(".pw") and nm.startswith("model.") else (nm if nm in ("model.0", "cpm.align") or nm.startswith("initial_stage.trunk.") else ("cpm" if nm == "cpm.conv" else None))
        if key is None or key not in taps:
            continue
        _within(eng.debug_layer_output(x, info["index"]), taps[key].numpy(), nm)
        checked += 1
    assert checked >= 15
    # every launch of a whole pass was an fp16 kernel
    layers = eng.layers()
    eng.debug_layer_output(x, layers[-1]["index"])
    seen = [eng.layer_variant(i["index"]) for i in layers]
    assert all(v and "bf16" not in v and "f16" in v for v in seen), seen
    got = net(x)
    for g, o in zip(got, outs):
        assert g.dtype == np.float32 and g.shape == tuple(o.shape)
        _within(g, o.numpy(), "stage output")


def test_f16_full_frame_batch_and_fused_post_is_exact_on_its_own_maps():
    net, sd = _calibrated()
    x = net_input(3, 368, 656, seed=0)
    outs = net(x)
    ref = net_ref.forward(sd, torch.from_numpy(x), 1)
    for o, r in zip(outs, ref):
        _within(o, r.numpy(), "stage output")
    res = net.engine.infer_poses(x, 4, demo=True)
    nk = 0
    for f in range(3):
        hu = post_ref.upsample_cubic(outs[-2][f].transpose(1, 2, 0), 4)
        pu = post_ref.upsample_cubic(outs[-1][f].transpose(1, 2, 0), 4)
        by_type, total = [], 0
        for k in range(18):
            total += post_ref.extract_keypoints(hu[:, :, k], by_type, total)
        ent, allk = post_ref.group_keypoints(by_type, pu, demo=True)
        e, a, c = res[f]
        assert np.array_equal(a, np.asarray(allk, dtype=np.float64).reshape(-1, 4))
        assert np.array_equal(e.reshape(-1, 20), np.asarray(ent, dtype=np.float64).reshape(-1, 20))
        nk += total
    assert nk > 100


def test_f16_skeletons_agree_with_the_fp32_oracle():
    m = _tool("f16_agreement").measure(4)
    for name, t in m["tensors"].items():
        sc = max(1.0, t["ref_max"])
        assert t["max_abs"] <= F16_TOL * sc and t["mean_abs"] <= F16_MEAN * sc, (name, t)
    assert m["oracle_kpts"] > 500
    assert m["oracle_kpts_matched"] >= 0.97 and m["kpts_matched_by_oracle"] >= 0.97, m
    for po, pf in m["poses_oracle_vs_net"]:
        assert abs(po - pf) <= 1, m["poses_oracle_vs_net"]


def test_f16_kernels_track_the_cpu_emulation():
    """The emulation (tools/f16_budget.py) that set the bars predicts the kernels' error: on the same weights and frames the HIP
    fp16 error against the fp32 oracle is within 0.5x - 2x of the emulated one."""
    net, sd = _calibrated()
    x = net_input(2, 368, 656, seed=300)
    outs = net(x)
    sdt = {k: (v if hasattr(v, "detach") else torch.as_tensor(np.asarray(v))) for k, v in sd.items()}
    xt = torch.from_numpy(x)
    ref = net_ref.forward(sdt, xt, 1)
    bb = _tool("f16_budget")._budget()
    bb.rb = lambda t: t.to(torch.float16).to(torch.float32)
    emu = bb.forward_emulated(sdt, xt, 1, set(bb.GROUPS))
    for i, (o, e, r) in enumerate(zip(outs, emu, ref)):
        r = r.numpy()
        hip_mean, emu_mean = np.abs(o - r).mean(), np.abs(e.numpy() - r).mean()
        hip_max, emu_max = np.abs(o - r).max(), np.abs(e.numpy() - r).max()
        assert 0.5 <= hip_mean / emu_mean <= 2.0, (i, hip_mean, emu_mean)
        assert 0.5 <= hip_max / emu_max <= 2.0, (i, hip_max, emu_max)


# ------------------------------------------------------------------------------------------ every bf16 variant, at fp16
_SD = {}


def _variant_sd():
    if "sd" not in _SD:
        _SD["sd"] = synth.make_state_dict(1, seed=1)
    return _SD["sd"]


def _variant_input(frame):
    n, h, w = frame
    return net_input(n, h, w, seed=400)


SWITCHES = sorted({k for r in vm.ROWS for k in r["env"]})
BF16_ROWS = [r for r in vm.ROWS if r["dtype"] == "bf16"]


def _engine(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(0, nref=1, dtype=_lib.F16)
    eng.load_state_dict(_variant_sd())
    for k in env:
        monkeypatch.delenv(k)
    return eng


def _tap(name, taps):
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


_REF64 = {}


def _ref64(frame):
    backbone_only = frame != vm.FRAME
    if frame not in _REF64:
        taps = {}
        net_ref.forward64(_variant_sd(), torch.from_numpy(_variant_input(frame)), 1, taps, stop_after="model.3" if backbone_only else None)
        _REF64[frame] = {k: v.numpy() for k, v in taps.items()}
    return _REF64[frame]


def _run(eng, x, names):
    idx = {l["name"]: l["index"] for l in eng.layers()}
    outs = {n: eng.debug_layer_output(x, idx[n]) for n in sorted(names, key=lambda n: idx[n])}
    last = max(idx[n] for n in names)
    eng.debug_layer_output(x, last)
    return outs, [(n, eng.layer_variant(idx[n])) for n in sorted(idx, key=idx.get)[:last + 1]]


_BASE = {}


@pytest.mark.parametrize("row", BF16_ROWS, ids=["%s-%s-%s" % (r["variant"], ",".join("%s=%s" % (k[4:], v) for k, v in sorted(r["env"].items())) or "default",
                                                r["layers"][0]) for r in BF16_ROWS])
def test_every_bf16_variant_has_an_f16_twin(monkeypatch, row):
    x = _variant_input(row["frame"])
    taps = _ref64(row["frame"])
    eng = _engine(monkeypatch, row["env"])
    outs, seen = _run(eng, x, row["layers"])
    var = dict(seen)
    assert all("bf16" not in v for _, v in seen), seen
    assert {nm: var[nm] for nm in row["layers"]} == {nm: _f16_twin(row["variant"]) for nm in row["layers"]}, seen
    for nm, got in outs.items():
        ref = _tap(nm, taps)
        assert got.shape == ref.shape
        _within(got, ref, nm)
    # the same input through the fp16 default kernels: the first layer whose kernel differs is one rounding step away at most
    env = {k: v for k, v in row["env"].items() if k in vm.STRUCTURAL}
    key = (tuple(sorted(env.items())), row["frame"])
    if key not in _BASE:
        _BASE[key] = _engine(monkeypatch, env)
    base = _BASE[key]
    _, bseen = _run(base, x, row["layers"])
    assert [n for n, _ in bseen] == [n for n, _ in seen]
    first = next((i for i, (a, b) in enumerate(zip(seen, bseen)) if a[1] != b[1]), None)
    if first is None:
        return
    nm = seen[first][0]
    if nm.endswith(".heads.0") and first + 1 < len(seen) and seen[first + 1][1] == seen[first][1]:
        nm = seen[first + 1][0]
    idx = {l["name"]: l["index"] for l in eng.layers()}
    a = eng.debug_layer_output(x, idx[nm]).astype(np.float64)
    b = base.debug_layer_output(x, idx[nm]).astype(np.float64)
    scale = max(1.0, float(np.abs(b).max()))
    assert np.all(np.abs(a - b) <= F16_STEP * np.maximum(np.abs(a), np.abs(b)) + F16_ABS * scale), (nm, float(np.abs(a - b).max()), scale)


# ------------------------------------------------------------------------------------------ batch, replicas, pipeline, multi-scale
def test_f16_batch32_frames_equal_single_frame_runs(monkeypatch):
    """Batch 32 at 368 x 656 takes the persistent window-resident 3x3 GEMM and the LDS-tiled front blocks; both engines force
    those kernels (LWP_GEMMH_AR_FORCE, LWP_DWPW_TILED) so that the single-frame runs use them too — then every pixel's
    summation order is the same and frames must agree bit for bit."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LWP_GEMMH_AR_FORCE", "1")
    monkeypatch.setenv("LWP_DWPW_TILED", "1")
    sd = synth.make_state_dict(1, seed=1)
    engs = []
    for _ in range(2):
        e = Engine(0, nref=1, dtype=_lib.F16)
        e.load_state_dict(sd)
        engs.append(e)
    monkeypatch.delenv("LWP_GEMMH_AR_FORCE")
    monkeypatch.delenv("LWP_DWPW_TILED")
    x = net_input(32, 368, 656, seed=700)
    big = engs[0].forward(x)
    idx = {l["name"]: l["index"] for l in engs[0].layers()}
    engs[0].debug_layer_output(x[:2], idx["cpm.conv"])
    assert engs[0].layer_variant(idx["cpm.conv"]).startswith("gemm_f16_ar<")
    for f in (0, 7, 31):
        one = engs[1].forward(x[f:f + 1])
        for b, o in zip(big, one):
            assert np.array_equal(b[f:f + 1], o), f


def test_f16_blob_replica_and_cross_dtype_import():
    net, sd = _calibrated()
    src = net.engine
    blob = torch.empty(src.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    src.export_weights(blob)
    rep = Engine(0, nref=1, dtype=_lib.F16)
    rep.import_weights(blob)
    x = net_input(2, 184, 328, seed=3)
    for a, b in zip(src.forward(x), rep.forward(x)):
        assert np.array_equal(a, b)
    pa, pb = src.infer_poses(x, 4, demo=True), rep.infer_poses(x, 4, demo=True)
    for fa, fb in zip(pa, pb):
        assert all(np.array_equal(u, v) for u, v in zip(fa, fb))
    # a blob of another dtype is refused in every direction
    bf = Engine(0, nref=1, dtype=_lib.BF16)
    bf.load_state_dict(sd)
    f32 = Engine(0, nref=1, dtype=_lib.F32)
    f32.load_state_dict(sd)
    bblob = torch.empty(bf.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    bf.export_weights(bblob)
    fblob = torch.empty(f32.weights_blob_bytes(), dtype=torch.uint8, device="cuda")
    f32.export_weights(fblob)
    with pytest.raises(ValueError):
        rep.import_weights(bblob)                  # bf16 -> fp16
    with pytest.raises(ValueError):
        bf.import_weights(blob)                    # fp16 -> bf16
    with pytest.raises(ValueError):
        rep.import_weights(fblob)                  # f32 -> fp16
    same_size = blob[:bblob.numel() + 16].clone()
    same_size[-16:] = 0                            # the right size without the tag
    with pytest.raises(ValueError):
        rep.import_weights(same_size)


def test_f16_pipeline_equals_serial_and_multiscale_step_tracks_the_oracle():
    net, sd = _calibrated()
    eng = net.engine
    frames = [torch.from_numpy(net_input(2, 368, 656, seed=10 * i)).cuda() for i in range(4)]
    serial = [eng.infer_poses(f, 4, demo=True) for f in frames]
    got = []
    for i, f in enumerate(frames):
        eng.pipeline_submit(f, i & 1)
        if i > 0:
            got.append(eng.pipeline_fetch((i - 1) & 1))
    got.append(eng.pipeline_fetch((len(frames) - 1) & 1))
    for a, b in zip(got, serial):
        for (ea, ka, ca), (eb, kb, cb) in zip(a, b):
            assert np.array_equal(ea, eb) and np.array_equal(ka, kb) and np.array_equal(ca, cb)
    from lwpose_amd.val import infer
    from oracle import preproc_ref
    img = synth.make_frames(1, 184, 240, seed0=5)[0]
    got_h, got_p = infer(net, img, [0.5, 1.0, 1.5], 368, 8)
    sdt = {k: (v if hasattr(v, "detach") else torch.as_tensor(np.asarray(v))) for k, v in sd.items()}
    ref_h, ref_p = preproc_ref.infer(sdt, 1, img, [0.5, 1.0, 1.5], 368, 8)
    assert got_h.shape == ref_h.shape and got_p.shape == ref_p.shape
    _within(got_h, ref_h, "multi-scale heat-maps")
    _within(got_p, ref_p, "multi-scale PAFs")
