"""fp16 against bf16 storage of the conv stack, emulated on the CPU: the table of DESIGN.md section 4a.

Runs tools/bf16_budget.py's emulation (every rounding group active = what the HIP 16-bit path rounds) twice, once rounding to
bfloat16 and once to IEEE half, on the calibrated 368x656 workload (nref 1, frames seed 300..), and reports per dtype the
stage-output error against the fp32 oracle (max / mean abs over scale = max(1, max|oracle|)), the key-point agreement through
the oracle's post-processing, the pose counts and the largest magnitude that was rounded (fp16 overflows beyond 65504).
Needs no GPU; tests/test_gpu_f16.py pins the HIP fp16 kernels to the fp16 row.

    python tools/f16_budget.py [frames]
"""
import importlib.util
import json
import os
import sys

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


def _budget():
    spec = importlib.util.spec_from_file_location("bf16_budget", os.path.join(_HERE, "bf16_budget.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def measure(n_frames=4, dtypes=("bf16", "fp16")):
    """{dtype: evaluate() row + "largest_rounded"} for the emulated 16-bit path."""
    from lwpose_amd import synth, workload
    from oracle import net_ref
    bb = _budget()
    nref = 1
    sd = bb.calibrated_state(nref)
    sd = {k: (v if hasattr(v, "detach") else torch.as_tensor(v)) for k, v in sd.items()}
    x = torch.from_numpy(workload.normalized_input(synth.make_frames(n_frames, 368, 656, seed0=300)))
    ref = net_ref.forward(sd, x, nref)
    ref_post = [bb.oracle_post(ref[-2][f].numpy(), ref[-1][f].numpy()) for f in range(n_frames)]
    out = {}
    for dt in dtypes:
        seen = [0.0]

        def rb(t, _ty=_TYPES[dt]):
            seen[0] = max(seen[0], float(t.abs().max()))
            return t.to(_ty).to(torch.float32)
        bb.rb = rb                                   # forward_emulated looks the rounding up at call time
        row = bb.evaluate(sd, x, nref, set(bb.GROUPS), ref, ref_post)
        row["largest_rounded"] = seen[0]
        out[dt] = row
    return out


def main():
    n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    rows = measure(n_frames)
    print("| emulated path | max-abs / scale (out0..out3) | mean-abs / scale (out2) | key-points matched (oracle->x / x->oracle) "
          "| poses oracle/x per frame | largest rounded magnitude |", file=sys.stderr)
    print("|---|---|---|---|---|---|", file=sys.stderr)
    for dt, r in rows.items():
        t = r["tensors"]
        print("| %s | %s | %.5f | %.3f / %.3f | %s | %.1f |" % (
            dt, " / ".join("%.4f" % t["out%d" % i]["max_abs_over_scale"] for i in range(4)), t["out2"]["mean_abs_over_scale"],
            r["oracle_kpts_matched"], r["emulated_kpts_matched"], ", ".join("%d/%d" % p for p in r["poses_oracle_vs_emulated"]),
            r["largest_rounded"]), file=sys.stderr)
    print(json.dumps({"frames": n_frames, "workload": "calibrated 368x656, nref 1, frames seed 300..", "rows": rows}))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(_HERE))
    main()
