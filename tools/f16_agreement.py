"""What the fp16 conv stack (LWP_F16) changes against the fp32 CPU oracle on the calibrated 368x656 workload: the measurement of
tools/bf16_agreement.py (same frames, same matching) run on the fp16 network.  Prints one JSON object; tests/test_gpu_f16.py
holds it to the fp16 bars.

    python tools/f16_agreement.py [frames]
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth, workload  # noqa: E402
from oracle import net_ref  # noqa: E402

_spec = importlib.util.spec_from_file_location("bf16_agreement", os.path.join(_HERE, "bf16_agreement.py"))
_agr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_agr)


def measure(n_frames=4, seed0=300, dtype="fp16"):
    net, sd = workload.build_net(nref=1, seed=1, device=0, dtype=dtype)
    fr = synth.make_frames(n_frames, 368, 656, seed0=seed0)
    x = workload.normalized_input(fr)
    outs = net(x)
    ref = net_ref.forward(sd, torch.from_numpy(x), 1)
    tens = {}
    for i, (o, r) in enumerate(zip(outs, ref)):
        r = r.numpy()
        tens["out%d" % i] = {"max_abs": float(np.abs(o - r).max()), "mean_abs": float(np.abs(o - r).mean()), "ref_max": float(np.abs(r).max())}
    res = net.engine.infer_poses(x, 4, demo=True)
    h1 = t1 = h2 = t2 = 0
    poses = []
    for f in range(n_frames):
        ent, allk, counts = _agr.oracle_post(ref[-2][f].numpy(), ref[-1][f].numpy())
        e, a, c = res[f]
        ga, gb = _agr.by_type_lists(allk, counts), _agr.by_type_lists(a, c)
        u, v = _agr.match_fraction(ga, gb); h1 += u; t1 += v
        u, v = _agr.match_fraction(gb, ga); h2 += u; t2 += v
        poses.append((len(ent), len(e)))
    return {"frames": n_frames, "dtype": dtype, "tensors": tens, "oracle_kpts_matched": h1 / max(t1, 1),
            "kpts_matched_by_oracle": h2 / max(t2, 1), "oracle_kpts": t1, "kpts": t2, "poses_oracle_vs_net": poses}


if __name__ == "__main__":
    print(json.dumps(measure(int(sys.argv[1]) if len(sys.argv) > 1 else 4)))
