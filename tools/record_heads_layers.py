"""Records tests/golden/heads_f32_layers.npz: the outputs of the small-M fp32 stage-head pair at the frames and
configurations of tests/heads_cases.py (needs a GPU).

    python tools/record_heads_layers.py [OUT.npz]

Run it on the commit whose outputs are to be held (the parent of a kernel rewrite that must not move a bit);
tests/test_gpu_heads_fixture.py then compares every later build with the file, bit for bit.  Everything is run twice and the
two runs must agree before anything is written."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lwpose_amd  # noqa: E402,F401
from lwpose_amd import _lib, synth  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

import heads_cases as hc  # noqa: E402


def frame_input(frame):
    n, h, w = frame
    x = (synth.make_frames(n, h, w, seed0=400).astype(np.float32) - 128.0) * np.float32(1 / 256)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def make_engine(env, sd):
    for k in hc.SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = Engine(0, nref=1, dtype=_lib.F32)
    eng.load_state_dict(sd)
    for k in env:
        os.environ.pop(k)
    return eng


def same(a, b):
    return a.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run_case(eng, x, layers):
    """({what: output}, {layer: variant}); every output computed twice, the runs bit-equal."""
    idx = {l["name"]: l["index"] for l in eng.layers()}
    out, var = {}, {}
    for nm in layers:
        a = eng.debug_layer_output(x, idx[nm])
        var[nm] = eng.layer_variant(idx[nm])
        assert same(a, eng.debug_layer_output(x, idx[nm])), (nm, "second run differs")
        out[nm] = a
    first, second = eng.forward(x), eng.forward(x)
    assert len(first) == hc.N_OUTS
    for i, (a, b) in enumerate(zip(first, second)):
        assert same(a, b), ("out%d" % i, "second run differs")
        out["out%d" % i] = a
    return out, var


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "heads_f32_layers.npz")
    sd = synth.make_state_dict(1, seed=1)
    engines, results, variants = {}, {}, {}
    for frame, cfg, env, layers in hc.cases():
        if cfg not in engines:
            engines[cfg] = make_engine(env, sd)
        out, var = run_case(engines[cfg], frame_input(frame), layers)
        for what, a in out.items():
            results[hc.key(frame, cfg, what)] = a
            print("%-50s %-14s %s" % (hc.key(frame, cfg, what), var.get(what, ""), a.shape), flush=True)
        for nm, v in var.items():
            assert v == hc.VARIANT, (frame, cfg, nm, v)
            variants[hc.key(frame, cfg, nm)] = v
    np.savez_compressed(out_path, **hc.pack(results, variants))
    back, v2 = hc.unpack(np.load(out_path))
    assert v2 == variants and set(back) == set(results)
    assert all(same(back[k], results[k]) for k in results)
    print(os.path.getsize(out_path), out_path)


if __name__ == "__main__":
    main()
