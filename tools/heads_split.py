"""Where the time of `heads_f32_kernel<8>` goes at batch 1 (368 x 656, a 46 x 82 map): single-stream HIP-event time of the two
stage launches (initial stage: four hidden tiles per wave; refinement stage: one) with parts of the kernel compiled out.
Needs a library built with LWP_ABLATION=1 (the instantiations exist only there) and a GPU:

    LWP_ABLATION=1 python lightweight-human-pose-estimation.pytorch_amd/build.py --force
    python tools/heads_split.py

LWP_HEADS_DEBUG bits: 1 no pixel-row loads, 2 no weight requests, 4 no MFMAs, 8 no reduction + epilogue.  One child process
per setting (the switch is read once per handle)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import os, sys, json
sys.path.insert(0, %r)
import lwpose_amd
from lwpose_amd import workload
net, _ = workload.build_net(1, 1, 0, "fp32", 368, 656, calibrate=False)
eng = net.engine
names = {l["name"]: l["index"] for l in eng.layers()}
out = {nm: eng.time_layer(names[nm], 1, 368, 656, 200) * 1e3 for nm in sys.argv[1:]}
print("RESULT " + json.dumps(out))
''' % ROOT
LAYERS = [("initial_stage.heads.0", "hidden 2 x 512"), ("refinement_stages.0.heads.0", "hidden 2 x 128")]
CFGS = [("full", 0), ("no x", 1), ("no W", 2), ("no MFMA", 4), ("no epi", 8), ("epi only", 7), ("launch", 15)]


def main():
    tab = {}
    for name, d in CFGS:
        env = dict(os.environ)
        env.pop("LWP_HEADS_DEBUG", None)
        if d:
            env["LWP_HEADS_DEBUG"] = str(d)
        r = subprocess.run([sys.executable, "-c", CHILD] + [l for l, _ in LAYERS], capture_output=True, text=True, env=env, timeout=120)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(name, (r.stderr or r.stdout)[-300:])
            return 1                                   # nothing more is started after a failed child
        tab[name] = json.loads(line[0][7:])
    print("%-30s %-16s" % ("layer (us)", "form") + "".join("%10s" % c[0] for c in CFGS))
    for nm, form in LAYERS:
        print("%-30s %-16s" % (nm, form) + "".join("%10.2f" % tab[c[0]][nm] for c in CFGS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
