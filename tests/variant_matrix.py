"""Kernel variant table: every template instantiation the launchers can pick, the ``LWP_*`` environment that forces it,
the layers it runs on and the exact ``layer_variant()`` string it must record.

Plain data (no torch, no GPU): tests/test_variant_closure.py checks it against the ``*_CASE(...)`` lists and launch
branches of the HIP sources on any machine; tests/test_kernel_variants.py runs every row on the GPU against the float64
oracle.  A new kernel configuration without a row here (or an ``UNREACHABLE`` entry) fails ``pytest -m "not gpu"``.

Geometry of the network rows: 2 x 3 x 91 x 149 frames -> maps of 46 x 75 (model.0, model.1), 23 x 38 (model.2, model.3) and
12 x 19 (model.4 on: M = 456 pixels, no multiple of any tile, tiles straddle the two frames).  At that size every launcher
heuristic takes its small-problem branch, so each row names the switch that forces its instantiation.

Row fields:
  family   kernel family (one launcher)
  env      LWP_* switches set before lwp_create (read once per handle)
  dtype    "fp32" | "bf16"
  layers   engine layer names the row checks
  variant  the exact layer_variant() string every one of those layers records (None: kernels that record none)
  frame    (N, H, W) of the input, when not the default 2 x 91 x 149
"""

FRAME = (2, 91, 149)

# engine switches that change the layer list (not a kernel choice): the baseline engine a row is compared with keeps them
STRUCTURAL = ("LWP_FUSE_DWPW", "LWP_FUSE_HEADS", "LWP_MERGE_HEADS")

PW_LAYERS = ["cpm.align",                                # 512 -> 128, the first 1x1 GEMM (input identical to the default engine's)
             "refinement_stages.0.trunk.0.initial",      # 185 -> 128 (cin_pad 192: six 32-channel blocks, uneven split-K at KS = 4)
             "refinement_stages.0.trunk.1.initial"]      # 128 -> 128 (four blocks: KS = 8 leaves four K groups without blocks)
C3_LAYERS = ["cpm.conv",                                 # the first dense 3x3
             "initial_stage.trunk.0",
             "refinement_stages.0.trunk.0.trunk.0",
             "refinement_stages.0.trunk.0.trunk.1"]      # dilation 2 + residual

ROWS = []


def _row(family, env, dtype, layers, variant, frame=None):
    ROWS.append(dict(family=family, env=dict(env), dtype=dtype, layers=list(layers), variant=variant, frame=frame or FRAME))


# ---------------------------------------------------------------- f32 implicit GEMM (dispatch_gemm): AR_CASE, WP_CASE, GEMM_CASE
AR_CFG = [(64, 1), (64, 2), (64, 4), (32, 4), (32, 8)]
WP_CFG = [(64, 1), (64, 2), (64, 4), (64, 8), (32, 4), (32, 8)]
GEMM_CFG = [(32, 64, 1), (32, 64, 2), (32, 64, 4), (64, 64, 1), (64, 64, 2), (64, 64, 4), (64, 128, 1), (64, 128, 2),
            (128, 128, 1), (32, 32, 4), (32, 32, 8)]
for bn, ks in AR_CFG:
    _row("gemm_ar", {"LWP_GEMM_PW": "32,%d,%d" % (bn, ks)}, "fp32", PW_LAYERS, "gemm_ar<%d,%d,1>" % (bn, ks))
    _row("gemm_ar", {"LWP_GEMM_C3": "32,%d,%d" % (bn, ks)}, "fp32", C3_LAYERS, "gemm_ar<%d,%d,3>" % (bn, ks))
for bn, ks in WP_CFG:
    _row("gemm_wp", {"LWP_GEMM_WP": "1", "LWP_GEMM_PW": "32,%d,%d" % (bn, ks)}, "fp32", PW_LAYERS, "gemm_wp<%d,%d,1>" % (bn, ks))
    _row("gemm_wp", {"LWP_GEMM_WP": "1", "LWP_GEMM_C3": "32,%d,%d" % (bn, ks)}, "fp32", C3_LAYERS, "gemm_wp<%d,%d,3>" % (bn, ks))
for bm, bn, ks in GEMM_CFG:
    _row("gemm", {"LWP_GEMM_WP": "0", "LWP_GEMM_PW": "%d,%d,%d" % (bm, bn, ks)}, "fp32", PW_LAYERS, "gemm<%d,%d,%d,1>" % (bm, bn, ks))
    _row("gemm", {"LWP_GEMM_WP": "0", "LWP_GEMM_C3": "%d,%d,%d" % (bm, bn, ks)}, "fp32", C3_LAYERS, "gemm<%d,%d,%d,3>" % (bm, bn, ks))
# unfused stage heads: two GEMMs, the second with cout 57 < cout_pad 64 (the heuristic's own picks, and forced ones)
_HEADS_GEMM_A = ["initial_stage.heads.0", "refinement_stages.0.heads.0", "refinement_stages.0.heads.1"]
_row("gemm_ar", {"LWP_FUSE_HEADS": "0"}, "fp32", _HEADS_GEMM_A, "gemm_ar<64,4,1>")
_row("gemm_ar", {"LWP_FUSE_HEADS": "0"}, "fp32", ["initial_stage.heads.1"], "gemm_ar<32,8,1>")
_row("gemm_ar", {"LWP_FUSE_HEADS": "0", "LWP_GEMM_PW": "32,32,4"}, "fp32", ["initial_stage.heads.1", "refinement_stages.0.heads.1"], "gemm_ar<32,4,1>")
_row("gemm_wp", {"LWP_FUSE_HEADS": "0", "LWP_GEMM_WP": "1", "LWP_GEMM_PW": "32,32,8"}, "fp32", ["initial_stage.heads.1", "refinement_stages.0.heads.1"], "gemm_wp<32,8,1>")
_row("gemm", {"LWP_FUSE_HEADS": "0", "LWP_GEMM_WP": "0", "LWP_GEMM_PW": "64,64,2"}, "fp32", ["initial_stage.heads.1", "refinement_stages.0.heads.1"], "gemm<64,64,2,1>")

# ---------------------------------------------------------------- stem (launch_stem_t): ty x wl, both dtypes
STEM_FORMS = [(16, 0), (8, 0), (4, 0), (4, 1), (2, 0), (2, 1)]
for dt in ("fp32", "bf16"):
    for ty, wl in STEM_FORMS:
        _row("stem", {"LWP_STEM_TY": str(ty), "LWP_STEM_WL": str(wl)}, dt, ["model.0"], "stem<ty=%d,wl=%d>" % (ty, wl))

# ---------------------------------------------------------------- stand-alone depthwise (launch_dw / try_dw_tiled), f32 only
_DW = {"LWP_FUSE_DWPW": "0", "LWP_DW_TILED": "1"}
_row("dw_tiled", _DW, "fp32", ["model.1.dw"], "dw_tiled<cc=32,s=1,d=1,ph=16>")
_row("dw_tiled", dict(_DW, LWP_DW_PH="8"), "fp32", ["model.1.dw"], "dw_tiled<cc=32,s=1,d=1,ph=8>")
_row("dw_tiled", _DW, "fp32", ["model.2.dw", "model.4.dw"], "dw_tiled<cc=64,s=2,d=1,ph=8>")
_row("dw_tiled", _DW, "fp32", ["model.3.dw", "model.5.dw", "model.6.dw", "cpm.trunk.0.dw", "cpm.trunk.2.dw"], "dw_tiled<cc=64,s=1,d=1,ph=8>")
_row("dw_tiled", dict(_DW, LWP_DW_PH="16"), "fp32", ["model.3.dw", "cpm.trunk.1.dw"], "dw_tiled<cc=64,s=1,d=1,ph=16>")
_row("dw_tiled", _DW, "fp32", ["model.7.dw"], "dw_tiled<cc=64,s=1,d=2,ph=8>")
_row("dw_tiled", dict(_DW, LWP_DW_PH="16"), "fp32", ["model.7.dw"], "dw_tiled<cc=64,s=1,d=2,ph=16>")
_row("dw_tiled", _DW, "fp32", ["model.8.dw", "model.11.dw"], "dw_tiled<cc=128,s=1,d=1,ph=8>")
_row("dw_tiled", dict(_DW, LWP_DW_PH="16"), "fp32", ["model.8.dw"], "dw_tiled<cc=128,s=1,d=1,ph=16>")
_row("dw_tiled", dict(_DW, LWP_DW_CC="128"), "fp32", ["model.3.dw"], "dw_tiled<cc=128,s=1,d=1,ph=8>")
_row("dw_tiled", dict(_DW, LWP_DW_CC="128"), "fp32", ["model.7.dw"], "dw_tiled<cc=128,s=1,d=2,ph=8>")
_row("dw_tiled", dict(_DW, LWP_DW_CC="128", LWP_DW_PH="16"), "fp32", ["model.7.dw"], "dw_tiled<cc=128,s=1,d=2,ph=16>")
_row("dw", {"LWP_FUSE_DWPW": "0", "LWP_DW_TILED": "0"}, "fp32", ["model.1.dw", "model.2.dw", "model.7.dw", "cpm.trunk.0.dw"], "dw<px=1>")
# dw<px=2>: the heuristic takes it at pixels * C / 4 >= 2^20 (one 720 x 1280 frame: model.1.dw is 360 x 640 x 32; backbone taps
# only), LWP_DW_PX=2 at every size.  At the default frame: Wo = 75 (model.1) and 19 (model.4 on) are odd, so the last thread of a
# row stores one pixel of its pair; model.2 / model.4 have stride 2, model.7 dilation 2, cpm.trunk.0 ELU
_row("dw", {"LWP_FUSE_DWPW": "0", "LWP_DW_TILED": "0"}, "fp32", ["model.1.dw", "model.3.dw"], "dw<px=2>", frame=(1, 720, 1280))
_row("dw", {"LWP_FUSE_DWPW": "0", "LWP_DW_TILED": "0", "LWP_DW_PX": "2"}, "fp32",
     ["model.1.dw", "model.2.dw", "model.4.dw", "model.7.dw", "cpm.trunk.0.dw"], "dw<px=2>")

# ---------------------------------------------------------------- f32 fused depthwise + pointwise (launch_dwpw): DP_CASE(bm, waves)
# waves per workgroup = cout / 32 unless LWP_DWPW_NW splits the columns: model.1 -> 2, model.2/3 + cpm.trunk -> 4, model.4/5 -> 8, model.6..11 -> 16
_NW_LAYERS = {2: ["model.1.pw"], 4: ["model.2.pw", "model.3.pw", "cpm.trunk.0.pw", "cpm.trunk.2.pw"], 8: ["model.4.pw", "model.5.pw"],
              16: ["model.6.pw", "model.7.pw", "model.11.pw"]}
for bm in (16, 32, 64):
    for nw, lay in _NW_LAYERS.items():
        _row("dwpw", {"LWP_DWPW_BM": str(bm)}, "fp32", lay, "dwpw<%d,%d>" % (bm, nw))
_row("dwpw", {"LWP_DWPW_BM": "32", "LWP_DWPW_NW": "2"}, "fp32", ["model.3.pw", "model.7.pw"], "dwpw<32,2>")
_row("dwpw", {"LWP_DWPW_BM": "64", "LWP_DWPW_NW": "4"}, "fp32", ["model.5.pw", "model.7.pw"], "dwpw<64,4>")
_row("dwpw", {"LWP_DWPW_BM": "16", "LWP_DWPW_NW": "8"}, "fp32", ["model.8.pw"], "dwpw<16,8>")
_row("dwpw_pipe", {"LWP_DWPW_PIPE": "1"}, "fp32", ["model.6.pw"], "dwpw_pipe<256>")
_row("dwpw_pipe", {"LWP_DWPW_PIPE": "1"}, "fp32", ["model.8.pw", "model.11.pw"], "dwpw_pipe<512>")
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "fp32", ["model.1.pw"], "dwpw_tiled<f32,32,64,s=1>")
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "fp32", ["model.2.pw"], "dwpw_tiled<f32,64,128,s=2>")
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "fp32", ["model.3.pw"], "dwpw_tiled<f32,128,128,s=1>")

# ---------------------------------------------------------------- bf16 fused depthwise + pointwise (launch_dwpw_bf16): DPH_CASE, DPH_DIL2
for bm in (16, 32, 64, 128):
    for nw, lay in _NW_LAYERS.items():
        lay = [l for l in lay if l != "model.7.pw"]
        _row("dwpw_bf16", {"LWP_DWPW_BM": str(bm)}, "bf16", lay, "dwpw_bf16<%d,%d,dil=1>" % (64 if bm == 128 and nw < 4 else bm, nw))
    _row("dwpw_bf16", {"LWP_DWPW_BM": str(bm)}, "bf16", ["model.7.pw"], "dwpw_bf16<%d,16,dil=2>" % bm)
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "bf16", ["model.1.pw"], "dwpw_tiled<bf16,32,64,s=1>")
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "bf16", ["model.2.pw"], "dwpw_tiled<bf16,64,128,s=2>")
_row("dwpw_tiled", {"LWP_DWPW_TILED": "1"}, "bf16", ["model.3.pw", "cpm.trunk.0.pw", "cpm.trunk.2.pw"], "dwpw_tiled<bf16,128,128,s=1>")
_row("dwpw_bf16_pp", {"LWP_DWPW_PP": "1"}, "bf16", ["model.5.pw"], "dwpw_bf16_pp<2,dil=1>")
_row("dwpw_bf16_pp", {"LWP_DWPW_PP": "1"}, "bf16", ["model.6.pw", "model.8.pw"], "dwpw_bf16_pp<4,dil=1>")
_row("dwpw_bf16_pp", {"LWP_DWPW_PP": "1"}, "bf16", ["model.7.pw"], "dwpw_bf16_pp<4,dil=2>")

# ---------------------------------------------------------------- fused stage heads
_HEADS = ["initial_stage.heads.1", "refinement_stages.0.heads.1"]
_row("heads_f32", {}, "fp32", _HEADS, "heads_f32<8>")
_row("heads_f32", {"LWP_HEADS_F32_MAXM": "16"}, "fp32", _HEADS, "heads_f32_lds<2>")
_row("heads_bf16", {}, "bf16", _HEADS, "heads_bf16<1>")
_row("heads_bf16", {"LWP_HEADS_RM": "2"}, "bf16", _HEADS, "heads_bf16<2>")

# ---------------------------------------------------------------- bf16 implicit GEMM: GH_CASE (shared tile), GAR_CASE (window resident)
GH_CFG = [(128, 128, 2, 2), (128, 64, 2, 1), (64, 64, 1, 1), (256, 128, 2, 2), (128, 128, 2, 1), (128, 128, 1, 1), (128, 64, 1, 1), (256, 128, 2, 1)]
for cfg in GH_CFG:
    _row("gemm_bf16", {"LWP_GEMMH": "%d,%d,%d,%d" % cfg}, "bf16", ["cpm.align", "cpm.conv", "refinement_stages.0.trunk.0.initial",
                                                                  "refinement_stages.0.trunk.0.trunk.1"], "gemm_bf16<%d,%d,%d,%d>" % cfg)
_GAR = {"LWP_GEMMH_AR_FORCE": "1"}
_GAR_PLAIN = ["cpm.conv", "initial_stage.trunk.2", "refinement_stages.0.trunk.0.trunk.0", "refinement_stages.0.trunk.4.trunk.1"]
_row("gemm_bf16_ar", _GAR, "bf16", _GAR_PLAIN, "gemm_bf16_ar<256,4,2,3>")
# the dilation-2 3x3 of refinement blocks 0..3 carries the next block's 128 -> 128 initial 1x1 in its epilogue when that 1x1 runs
# in the same pass; the folded 1x1 records the same string and its output is the folded kernel's
_row("gemm_bf16_ar", _GAR, "bf16", ["refinement_stages.0.trunk.1.initial", "refinement_stages.0.trunk.3.initial"], "gemm_bf16_ar<256,4,2,3>+1x1")
_row("gemm_bf16_ar", dict(_GAR, LWP_GEMMH_FOLD="0"), "bf16", ["refinement_stages.0.trunk.0.trunk.1", "refinement_stages.0.trunk.2.trunk.1"],
     "gemm_bf16_ar<256,4,2,3>")
_row("gemm_bf16_ar", dict(_GAR, LWP_GEMMH_PERSIST="0"), "bf16", ["cpm.conv", "refinement_stages.0.trunk.4.trunk.1"], "gemm_bf16_ar<256,4,2,3>")
for cfg in [(128, 2, 2, 3), (128, 4, 2, 3)]:
    _row("gemm_bf16_ar", dict(_GAR, LWP_GEMMH_AR="%d,%d,%d,%d" % cfg), "bf16", ["cpm.conv", "initial_stage.trunk.0",
                                                                             "refinement_stages.0.trunk.0.trunk.1"], "gemm_bf16_ar<%d,%d,%d,%d>" % cfg)

# ---------------------------------------------------------------- exact kernels (no variant string): compared bit for bit with oracle/post_ref
UPSAMPLE_ROWS = [dict(family="upsample", env={}, ratio=4, kernel="upsample_tiled_kernel<4>"),
                 dict(family="upsample", env={}, ratio=8, kernel="upsample_tiled_kernel<8>"),
                 dict(family="upsample", env={"LWP_UPSAMPLE_TILED": "0"}, ratio=4, kernel="upsample_kernel"),
                 dict(family="upsample", env={"LWP_UPSAMPLE_TILED": "0"}, ratio=8, kernel="upsample_kernel")]
# fused multi-scale step: forced tile widths (the kernel takes 8..40); 11, 26 and 40 divide none of the destination widths used
MS_TX = [8, 11, 16, 26, 40]

# instantiations no layer of any supported geometry reaches (kept in the sources; deleting them is a separate change)
UNREACHABLE = {
    "DT_CASE(32,1,2)": "only model.1.dw has 32 channels, and it has dilation 1",
    "DT_CASE(32,2,1)": "only model.1.dw has 32 channels, and it has stride 1",
    "dwpw_bf16_pp<2,dil=2>": "the only dilation-2 block (model.7) has 512 outputs",
}
