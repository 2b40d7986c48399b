"""Cost of the generic grouping kernels, recorded (not gated): at 368x656, fp32, batch 1 and 32, on calibrated synthetic
weights, for the COCO skeleton on the specialised kernels, the COCO skeleton under LWP_POST_GENERIC=1 (same network, same
maps), and the guide5 / hand21 / coco_dense skeletons (networks with num_heatmaps = K + 1, num_pafs = 2 L).  Per
configuration: the post-processing class time of one pass (lwp_profile_classes class 4, averaged over --reps passes) and
the frames/s of lwp_time_pipeline (network + post-processing, --iters back-to-back passes).  Writes one JSON file.

    python tools/skeleton_bench.py [--out profiles/skeleton/skeleton_post.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth, workload  # noqa: E402
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet  # noqa: E402
from lwpose_amd.modules.load_state import load_state  # noqa: E402
import skeleton_cases as sc  # noqa: E402


def custom_net(NH, NP, kpts, pafs, H, W, generic=False):
    old = os.environ.get("LWP_POST_GENERIC")
    if generic:
        os.environ["LWP_POST_GENERIC"] = "1"
    try:
        if NH == 19 and NP == 38 and kpts is None:
            net, _ = workload.build_net(nref=1, seed=1, device=0, height=H, width=W)
            return net
        sd = synth.make_state_dict(1, seed=1, num_heatmaps=NH, num_pafs=NP)
        net = PoseEstimationWithMobileNet(num_refinement_stages=1, num_heatmaps=NH, num_pafs=NP)
        load_state(net, {"state_dict": sd})
        net.eval().cuda()
        outs = net(workload.normalized_input(synth.make_frames(1, H, W, seed0=0)))
        sd = synth.calibrate_heads(sd, outs[-2][0], outs[-1][0], 1)
        load_state(net, {"state_dict": sd})
        net.cuda()
        net.engine.set_skeleton(kpts, pafs, NH - 1)
        return net
    finally:
        if generic:
            if old is None:
                del os.environ["LWP_POST_GENERIC"]
            else:
                os.environ["LWP_POST_GENERIC"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=368)
    ap.add_argument("--width", type=int, default=656)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton", "skeleton_post.json"))
    args = ap.parse_args()
    H, W = args.height, args.width
    configs = [("coco_specialised", 19, 38, None, None, False), ("coco_generic", 19, 38, None, None, True),
               ("guide5", 6, 8, sc.GUIDE5_KPTS, sc.GUIDE5_PAFS, False), ("hand21", 22, 40, sc.HAND21_KPTS, sc.HAND21_PAFS, False),
               ("coco_dense", 19, 2 * len(sc.DENSE_KPTS), sc.DENSE_KPTS, sc.DENSE_PAFS, False)]
    rows = []
    for name, NH, NP, kpts, pafs, generic in configs:
        net = custom_net(NH, NP, kpts, pafs, H, W, generic)
        eng = net.engine
        for batch in (1, 32):
            x = torch.from_numpy(workload.normalized_input(synth.make_frames(batch, H, W, seed0=0))).cuda(0)
            res = eng.infer_poses(x, 4, demo=True)
            cls = eng.profile_classes(x, reps=args.reps)
            eng.time_pipeline(x, 3)
            ms = eng.time_pipeline(x, args.iters)
            row = {"config": name, "batch": batch, "num_kpt_types": eng.skeleton["num_kpt_types"],
                   "num_limbs": len(eng.skeleton["limb_kpts"]), "post_ms": cls["post"]["ms"], "post_launches": cls["post"]["launches"],
                   "frames_per_s": batch * args.iters / (ms / 1000.0), "poses_frame0": int(len(res[0][0])),
                   "kpts_frame0": int(res[0][2].sum())}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del net, eng
        torch.cuda.synchronize()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"height": H, "width": W, "dtype": "fp32", "reps": args.reps, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
