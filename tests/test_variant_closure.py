"""Closure of tests/variant_matrix.py over the HIP sources (CPU only).

Every configuration a launcher can instantiate (the ``*_CASE(...)`` lists, the stem / depthwise / heads / fused-block /
up-sample launch branches) must be a row of the variant table or listed in ``UNREACHABLE`` with a reason, and every variant
string of the table must be one the launchers' ``LWP_VARIANT`` formats can print.  A new kernel configuration without a
test row fails here."""
import os
import re

import variant_matrix as vm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "lightweight-human-pose-estimation.pytorch_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _cases(text, macro, nargs):
    """Numeric argument tuples of every ``MACRO(a, b, ...)`` use (the #define line has parameter names and is skipped)."""
    pat = r"\b%s\(%s\)" % (macro, r",\s*".join([r"(\d+)"] * nargs))
    return [tuple(int(v) for v in (m if nargs > 1 else (m,))) for m in re.findall(pat, text)]


def _body(text, signature):
    """Source of the function starting at ``signature`` up to its closing brace at column 0."""
    i = text.index(signature)
    return text[i:text.index("\n}\n", i)]


def expected_instantiations():
    """{key: [variant strings]} of every configuration the launchers can instantiate."""
    f32, h16, tl, post = _src("net_kernels.hip"), _src("net_kernels_bf16.hip"), _src("net_kernels_tiled.hip"), _src("post_kernels.hip")
    out = {}
    disp = _body(f32, "static hipError_t dispatch_gemm(")
    for bn, ks in _cases(disp, "AR_CASE", 2):
        out["AR_CASE(%d,%d)" % (bn, ks)] = ["gemm_ar<%d,%d,%d>" % (bn, ks, k) for k in (1, 3)]
    for bn, ks in _cases(disp, "WP_CASE", 2):
        out["WP_CASE(%d,%d)" % (bn, ks)] = ["gemm_wp<%d,%d,%d>" % (bn, ks, k) for k in (1, 3)]
    for bm, bn, ks in _cases(disp, "GEMM_CASE", 3):
        out["GEMM_CASE(%d,%d,%d)" % (bm, bn, ks)] = ["gemm<%d,%d,%d,%d>" % (bm, bn, ks, k) for k in (1, 3)]
    # stem: one launch branch per (tile height, weights-through-LDS) form; both dtypes share the template
    stem = _body(f32, "static hipError_t launch_stem_t(")
    forms = re.findall(r"if \(ty == (\d+)( && wl)?\) hipLaunchKernelGGL\(\(stem_kernel<", stem)
    assert len(forms) >= 6, forms
    assert "launch_stem_t<false>" in f32 and "launch_stem_t<true>" in f32
    for ty, wl in forms:
        out["stem<ty=%s,wl=%d>" % (ty, 1 if wl else 0)] = [("stem<ty=%s,wl=%d>" % (ty, 1 if wl else 0), dt) for dt in ("fp32", "bf16")]
    # stand-alone depthwise: tiled (channels per workgroup, stride, dilation) x patch rows (16 only at stride 1), per-thread kernel
    for cc, s, d in _cases(_body(f32, "static hipError_t try_dw_tiled("), "DT_CASE", 3):
        out["DT_CASE(%d,%d,%d)" % (cc, s, d)] = ["dw_tiled<cc=%d,s=%d,d=%d,ph=%d>" % (cc, s, d, ph) for ph in ((8, 16) if s == 1 else (8,))]
    for px in re.findall(r"hipLaunchKernelGGL\(dw_kernel<(\d+)>", _body(f32, "hipError_t launch_dw(")):
        out["dw_kernel<%s>" % px] = ["dw<px=%s>" % px]
    # fused depthwise + pointwise, f32
    for bm, nw in _cases(_body(f32, "hipError_t launch_dwpw("), "DP_CASE", 2):
        out["DP_CASE(%d,%d)" % (bm, nw)] = ["dwpw<%d,%d>" % (bm, nw)]
    for c in re.findall(r"launch_dwpw_pipe_t<(\d+)>", _body(f32, "static hipError_t try_dwpw_pipe(")):
        out["dwpw_pipe_t<%s>" % c] = ["dwpw_pipe<%s>" % c]
    # fp32 stage heads: 16-pixel kernel and the LDS-staged pair above the M limit
    heads = _body(f32, "hipError_t launch_heads_f32(")
    out["heads_f32_kernel"] = ["heads_f32<%s>" % re.search(r"constexpr int NW = (\d+);", heads).group(1)]
    out["heads_f32_lds_kernel"] = ["heads_f32_lds<%s>" % re.search(r"constexpr int PT = (\d+);", heads).group(1)]
    # bf16 fused blocks
    dph = _body(h16, "hipError_t launch_dwpw_bf16(")
    for bm, nw in _cases(dph, "DPH_CASE", 2):
        out["DPH_CASE(%d,%d)" % (bm, nw)] = ["dwpw_bf16<%d,%d,dil=1>" % (bm, nw)]
    for (bm,) in _cases(dph, "DPH_DIL2", 1):
        out["DPH_DIL2(%d)" % bm] = ["dwpw_bf16<%d,16,dil=2>" % bm]
    for half, dil in re.findall(r"launch_dwpw_bf16_pp_t<(\d+), ACT_RELU, (\d+)>", _body(h16, "static hipError_t try_dwpw_bf16_pp(")):
        key = "dwpw_bf16_pp<%s,dil=%s>" % (half, dil)
        out[key] = [key]
    for rm in re.findall(r"launch_heads_bf16_t<(\d+)>", _body(h16, "hipError_t launch_heads_bf16(")):
        out["heads_bf16_t<%s>" % rm] = ["heads_bf16<%s>" % rm]
    # bf16 GEMMs: window-resident (and its folded-1x1 epilogue), shared-tile
    gar = _body(h16, "static hipError_t try_gemm_bf16_ar(")
    for cfg in _cases(gar, "GAR_CASE", 4):
        out["GAR_CASE(%d,%d,%d,%d)" % cfg] = ["gemm_bf16_ar<%d,%d,%d,%d>" % cfg]
    for fold in re.findall(r'LWP_VARIANT\(p, "(gemm_bf16_ar<[\d,]+>\+1x1)"\)', gar):
        out[fold] = [fold]
    for cfg in _cases(_body(h16, "hipError_t launch_gemm_bf16("), "GH_CASE", 4):
        out["GH_CASE(%d,%d,%d,%d)" % cfg] = ["gemm_bf16<%d,%d,%d,%d>" % cfg]
    # LDS-tiled fused blocks (both dtypes) and the bf16 ELU form
    tiled = _body(tl, "static hipError_t try_tiled(")
    for c, co, s, _ph in _cases(tiled, "TL_CASE", 4):
        out["TL_CASE(%d,%d,%d)" % (c, co, s)] = [("dwpw_tiled<%s,%d,%d,s=%d>" % (n, c, co, s), dt) for n, dt in (("f32", "fp32"), ("bf16", "bf16"))]
    for c, co, s in re.findall(r"launch_tiled_t<true, (\d+), (\d+), (\d+), \d+, ACT_ELU>", tiled):
        out["TL_ELU(%s,%s,%s)" % (c, co, s)] = [("dwpw_tiled<bf16,%s,%s,s=%s>" % (c, co, s), "bf16")]
    # up-sample (no variant string): the kernels launch_upsample can launch
    ups = _body(post, "hipError_t launch_upsample(")
    for k in re.findall(r"hipLaunchKernelGGL\((upsample(?:_tiled)?_kernel(?:<\d+>)?),", ups):
        out[k] = []
    return out


def _formats():
    fm = []
    for name in ("net_kernels.hip", "net_kernels_bf16.hip", "net_kernels_tiled.hip"):
        fm += re.findall(r'LWP_VARIANT\(p, "([^"]+)"', _src(name))
    return fm


def _fmt_regex(fmt):
    return re.compile(re.escape(fmt).replace("%d", r"-?\d+").replace("%s", r"[a-z0-9]+"))


def _table():
    return {(r["variant"], r["dtype"]) for r in vm.ROWS}


def test_every_instantiation_has_a_row_or_a_reason():
    inst = expected_instantiations()
    table = _table()
    variants = {v for v, _ in table}
    assert len(inst) >= 70, sorted(inst)
    missing = []
    for key, vs in inst.items():
        if key in vm.UNREACHABLE:
            continue
        if key.startswith("upsample"):
            if not any(u["kernel"] == key for u in vm.UPSAMPLE_ROWS):
                missing.append(key)
            continue
        for v in vs:
            if isinstance(v, tuple):
                if v in table or v[0] in vm.UNREACHABLE:
                    continue
                missing.append("%s (%s)" % v)
            elif v not in variants and v not in vm.UNREACHABLE:
                missing.append(v)
    assert not missing, "kernel configurations without a row in tests/variant_matrix.py: %s" % missing


def test_per_thread_depthwise_forms_are_forced_at_the_default_frame():
    """``LWP_DW_PX`` is parsed into ``Tuning`` and decides launch_dw's branch, and every dw_kernel<PX> has a row at the default
    frame (PX = 2: forced by the switch, with an odd output width among its layers) next to the workload-size row."""
    f32 = _src("net_kernels.hip")
    assert re.search(r'geti\("LWP_DW_PX", &t\.dw_px\)', _body(f32, "Tuning tuning_from_env("))
    assert "int dw_px = 0;" in _src("lwp_internal.h")
    body = _body(f32, "hipError_t launch_dw(")
    assert re.search(r"T\.dw_px == 1 \|\| T\.dw_px == 2 \? T\.dw_px == 2 :", body)
    pxs = set(re.findall(r"hipLaunchKernelGGL\(dw_kernel<(\d+)>", body))
    assert pxs == {"1", "2"}
    rows = [r for r in vm.ROWS if r["family"] == "dw"]
    for px in pxs:
        at_frame = [r for r in rows if r["variant"] == "dw<px=%s>" % px and r["frame"] == vm.FRAME]
        assert at_frame, px
        assert all(r["env"].get("LWP_DW_TILED") == "0" and r["env"].get("LWP_FUSE_DWPW") == "0" for r in at_frame)
    forced = [r for r in rows if r["variant"] == "dw<px=2>" and r["frame"] == vm.FRAME]
    assert all(r["env"].get("LWP_DW_PX") == "2" for r in forced)
    # widths of the default frame's maps (variant_matrix's header): model.1 has 75 columns, model.4 on 19
    assert any(l in ("model.1.dw", "model.4.dw", "model.7.dw", "cpm.trunk.0.dw") for r in forced for l in r["layers"])
    assert any(r["variant"] == "dw<px=2>" and r["frame"] == (1, 720, 1280) and "LWP_DW_PX" not in r["env"] for r in rows)


def test_unreachable_entries_name_real_instantiations_with_reasons():
    inst = expected_instantiations()
    known = set(inst) | {v if isinstance(v, str) else v[0] for vs in inst.values() for v in vs}
    table = {v for v, _ in _table()}
    for key, reason in vm.UNREACHABLE.items():
        assert key in known, key                       # a stale entry (the instantiation is gone) must go too
        assert isinstance(reason, str) and len(reason) > 10, key
        assert key not in table, key                   # listed as unreachable but forced by a row: one of them is wrong


def test_table_variants_match_the_launchers_formats():
    regs = [_fmt_regex(f) for f in _formats()]
    assert len(regs) >= 14
    for r in vm.ROWS:
        assert r["variant"] is not None and any(g.fullmatch(r["variant"]) for g in regs), r
    # and every format is exercised by some row (a new launcher with a variant string of its own needs rows)
    for f, g in zip(_formats(), regs):
        assert any(g.fullmatch(r["variant"]) for r in vm.ROWS), f


def test_table_is_well_formed():
    keys = set()
    for r in vm.ROWS:
        assert r["dtype"] in ("fp32", "bf16") and r["layers"] and all(k.startswith("LWP_") for k in r["env"]), r
        assert len(r["frame"]) == 3
        key = (tuple(sorted(r["env"].items())), r["dtype"], r["variant"], tuple(r["layers"]))
        assert key not in keys, r
        keys.add(key)
    # both ends of the forced multi-scale tile width and at least two widths that divide none of the tested map widths
    lo, hi = map(int, re.search(r"ms_tx >= (\d+) && h->tune\.ms_tx <= (\d+)", _src("capi.cpp")).groups())
    assert min(vm.MS_TX) == lo and max(vm.MS_TX) == hi
    assert sum(1 for t in vm.MS_TX if all(w % t for w in (150, 301, 328))) >= 2
    assert {u["ratio"] for u in vm.UPSAMPLE_ROWS} == {4, 8}
