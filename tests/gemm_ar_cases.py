"""Cases of the bit-for-bit fixture of the A-resident f32 GEMM convs (``gemm_ar_kernel``): tests/golden/gemm_ar_layers.npz.

Plain data and two small helpers shared by tools/record_gemm_layers.py (writes the fixture from a GPU run of the commit
whose outputs are to be held) and tests/test_gpu_gemm_ar_fixture.py (compares the current build with it).

Frames (N, H, W) -> map, and what each exercises in the kernel's index and bounds logic:
  (2, 91, 149) -> 12 x 19, M = 456: the map is narrower than the 34- / 36-row window segments, so a window wraps several image
                  rows; tiles straddle the two frames; the last tile is ragged
  (1, 8, 256)  -> 1 x 32: exactly one tile; H = 1, so every dy != 0 tap is outside the image
  (1, 24, 40)  -> 3 x 5, M = 15 < one tile: dilation 2 reaches outside on every side, first-tile window offsets are negative and
                  last-tile offsets run past M
"""
import json

import numpy as np

import variant_matrix as vm

BIG = (2, 91, 149)
SMALL = [(1, 8, 256), (1, 24, 40)]

TRUNK4 = "refinement_stages.0.trunk.4.trunk.1"             # dilation 2 + residual, the last block of the trunk
HEADS = ["initial_stage.heads.0", "initial_stage.heads.1"]  # unfused head pair: the second has cout 57 < cout_pad 64 and the NCHW split
FORCED = ["32,64,1", "32,64,2", "32,64,4", "32,32,4", "32,32,8"]

# (configuration name, LWP_* switches, layers) at the two small frames
CONFIGS = [("default", {}, vm.PW_LAYERS + vm.C3_LAYERS + [TRUNK4]),
           ("heads", {"LWP_FUSE_HEADS": "0"}, HEADS)]
for _c in FORCED:
    CONFIGS.append(("c3=" + _c, {"LWP_GEMM_C3": _c}, vm.C3_LAYERS + [TRUNK4]))
    CONFIGS.append(("pw=" + _c, {"LWP_GEMM_PW": _c}, vm.PW_LAYERS))
# the 456-pixel frame: the default engine, the uneven-K 1x1 (185 -> 128) and a dilation-2 3x3 with residual
BIG_LAYERS = ["refinement_stages.0.trunk.0.initial", "refinement_stages.0.trunk.0.trunk.1"]

SWITCHES = ["LWP_GEMM_C3", "LWP_GEMM_PW", "LWP_GEMM_WP", "LWP_FUSE_HEADS", "LWP_GEMM_DEBUG"]


def cases():
    """[(frame, configuration name, env, layers)]"""
    out = [(BIG, "default", {}, list(BIG_LAYERS))]
    for fr in SMALL:
        for name, env, layers in CONFIGS:
            out.append((fr, name, dict(env), list(layers)))
    return out


def key(frame, cfg, layer):
    return "%dx%dx%d|%s|%s" % (frame + (cfg, layer))


def pack(results, variants):
    """results {key: float32 array}, variants {key: str} -> dict for np.savez_compressed.  A forced configuration's array is
    stored as the XOR of its bits with the default configuration's same layer (summation order only: the high bytes are
    zero and compress away); everything is reconstructed exactly by unpack()."""
    out = {"variants": np.frombuffer(json.dumps(variants, sort_keys=True).encode(), dtype=np.uint8)}
    for k, a in results.items():
        fr, cfg, layer = k.split("|")
        base = results.get("|".join([fr, "default", layer]))
        a = np.ascontiguousarray(a, dtype=np.float32)
        if cfg != "default" and base is not None:
            out["x:" + k] = a.view(np.uint32) ^ np.ascontiguousarray(base, dtype=np.float32).view(np.uint32)
        else:
            out["f:" + k] = a
    return out


def unpack(npz):
    variants = json.loads(bytes(npz["variants"]).decode())
    res = {n[2:]: npz[n] for n in npz.files if n.startswith("f:")}
    for n in npz.files:
        if n.startswith("x:"):
            fr, cfg, layer = n[2:].split("|")
            res[n[2:]] = (npz[n] ^ res["|".join([fr, "default", layer])].view(np.uint32)).view(np.float32)
    return res, variants
