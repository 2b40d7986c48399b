"""Records tests/golden/gemm_ar_layers.npz: `debug_layer_output` of the f32 GEMM conv layers at the small frames of
tests/gemm_ar_cases.py, default engine and the forced forms that share `gemm_ar_kernel` (needs a GPU).

    python tools/record_gemm_layers.py [OUT.npz]

Run it on the commit whose outputs are to be held (the parent of a kernel rewrite that must not move a bit);
tests/test_gpu_gemm_ar_fixture.py then compares every later build with the file, bit for bit.  Each layer is run twice and the
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

import gemm_ar_cases as gc  # noqa: E402


def frame_input(frame):
    n, h, w = frame
    x = (synth.make_frames(n, h, w, seed0=400).astype(np.float32) - 128.0) * np.float32(1 / 256)
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def make_engine(env, sd):
    for k in gc.SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    eng = Engine(0, nref=1, dtype=_lib.F32)
    eng.load_state_dict(sd)
    for k in env:
        os.environ.pop(k)
    return eng


def run_case(eng, x, layers):
    """{layer: (output, variant)}; every layer run twice, the runs bit-equal."""
    idx = {l["name"]: l["index"] for l in eng.layers()}
    out = {}
    for nm in layers:
        a = eng.debug_layer_output(x, idx[nm])
        var = eng.layer_variant(idx[nm])
        b = eng.debug_layer_output(x, idx[nm])
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (nm, "second run differs")
        out[nm] = (a, var)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "gemm_ar_layers.npz")
    sd = synth.make_state_dict(1, seed=1)
    engines, results, variants = {}, {}, {}
    for frame, cfg, env, layers in gc.cases():
        if cfg not in engines:
            engines[cfg] = make_engine(env, sd)
        for nm, (a, var) in run_case(engines[cfg], frame_input(frame), layers).items():
            results[gc.key(frame, cfg, nm)] = a
            variants[gc.key(frame, cfg, nm)] = var
            print("%-60s %-18s %s" % (gc.key(frame, cfg, nm), var, a.shape), flush=True)
    np.savez_compressed(out_path, **gc.pack(results, variants))
    back, v2 = gc.unpack(np.load(out_path))
    assert v2 == variants and set(back) == set(results)
    assert all(np.array_equal(back[k].view(np.uint32), results[k].view(np.uint32)) for k in results)
    print(os.path.getsize(out_path), out_path)


if __name__ == "__main__":
    main()
