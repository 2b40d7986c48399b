"""Cases of the bit-for-bit fixture of the small-M fp32 stage-head kernel (``heads_f32_kernel``): tests/golden/heads_f32_layers.npz.

Plain data and two small helpers shared by tools/record_heads_layers.py (writes the fixture from a GPU run of the commit
whose outputs are to be held) and tests/test_gpu_heads_fixture.py (compares the current build with it).

Layers: ``initial_stage.heads.1`` (hidden 2 x 512: four hidden tiles per wave, the paired steps of the kernel's loop) and
``refinement_stages.0.heads.1`` (hidden 2 x 128: one tile per wave, the unpaired last step alone).

Frames (N, H, W) -> map, and what each exercises in the kernel's index and bounds logic:
  (1, 8, 256)  -> 1 x 32: exactly one pixel tile, both 16-pixel blocks full
  (1, 24, 40)  -> 3 x 5, M = 15: the second pixel block is wholly out of range and the first is ragged
  (2, 91, 149) -> 12 x 19, M = 456: the last tile holds 8 pixels and tiles straddle the two frames

Per frame and configuration two kinds of output are held: the NHWC window of the concat buffer that the pair writes
(``debug_layer_output`` of the two layers above) and the NCHW stage maps of an ordinary forward (keys ``out0`` .. ``out3``).

Configurations: the default engine, where the merged pair runs as ``heads_f32<8>``, and LWP_MERGE_HEADS=0.  The un-merged
graph has four separate head convs per stage and no ``.heads.1`` layer, so no pair is fused there and the kernel does not run:
that configuration holds the stage maps only (the GEMM kernels' outputs), with no variant to assert.
"""
import json

import numpy as np

FRAMES = [(1, 8, 256), (1, 24, 40), (2, 91, 149)]
LAYERS = ["initial_stage.heads.1", "refinement_stages.0.heads.1"]
VARIANT = "heads_f32<8>"
N_OUTS = 4                                                  # nref 1: heat / PAF maps of the initial and one refinement stage

# (configuration name, LWP_* switches, layers read through debug_layer_output)
CONFIGS = [("default", {}, LAYERS),
           ("unmerged", {"LWP_MERGE_HEADS": "0"}, [])]

SWITCHES = ["LWP_MERGE_HEADS", "LWP_FUSE_HEADS", "LWP_HEADS_F32_MAXM", "LWP_HEADS_F32_LDS", "LWP_HEADS_DEBUG"]


def cases():
    """[(frame, configuration name, env, layers)]"""
    return [(fr, name, dict(env), list(layers)) for fr in FRAMES for name, env, layers in CONFIGS]


def key(frame, cfg, what):
    return "%dx%dx%d|%s|%s" % (frame + (cfg, what))


def _window(results, k):
    """the concat window of a ``.heads.1`` layer from the stage maps of the same frame and configuration: [heat | PAF]"""
    fr, cfg, layer = k.split("|")
    o = 2 * LAYERS.index(layer)
    return np.concatenate([results["|".join([fr, cfg, "out%d" % i])] for i in (o, o + 1)], axis=1)


def _default(k):
    fr, _cfg, what = k.split("|")
    return "|".join([fr, "default", what])


def pack(results, variants):
    """results {key: float32 array}, variants {key: str} -> dict for np.savez_compressed.  The pair writes every value to the
    concat window and to a stage map: a window must equal its two maps bit for bit, and only the maps are stored.  A map of
    another configuration is stored as the XOR of its bits with the default configuration's (summation order only: the high
    bytes are zero and compress away); everything is reconstructed exactly by unpack()."""
    out = {"variants": np.frombuffer(json.dumps(variants, sort_keys=True).encode(), dtype=np.uint8)}
    for k, a in results.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        if k.split("|")[2] in LAYERS:
            assert np.array_equal(a.view(np.uint32), _window(results, k).view(np.uint32)), (k, "window and stage maps differ")
        elif k.split("|")[1] != "default":
            out["x:" + k] = a.view(np.uint32) ^ np.ascontiguousarray(results[_default(k)], dtype=np.float32).view(np.uint32)
        else:
            out["f:" + k] = a
    return out


def unpack(npz):
    variants = json.loads(bytes(npz["variants"]).decode())
    res = {n[2:]: npz[n] for n in npz.files if n.startswith("f:")}
    for n in npz.files:
        if n.startswith("x:"):
            res[n[2:]] = (npz[n] ^ res[_default(n[2:])].view(np.uint32)).view(np.float32)
    for k in variants:
        res[k] = _window(res, k)
    return res, variants
