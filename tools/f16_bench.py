"""fp16 against bf16 conv-stack throughput, in ONE process: both networks (calibrated, nref 1) on the same frames, batch 32 at
368x656 by default, the full pipelined pass of bench.py (network + post-processing, two result slots, poses fetched to the
host) timed in ALTERNATING blocks of --steps steps, so clock and thermal drift hit both dtypes alike.  Prints one JSON line:
the median frames/s of each dtype's blocks, every block's figure, and fp16 / bf16.

    python tools/f16_bench.py [--batch 32] [--steps 32] [--blocks 6] [--warmup 8]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import synth, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=368)
    ap.add_argument("--width", type=int, default=656)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=6, help="timed blocks per dtype")
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    x = torch.from_numpy(workload.normalized_input(synth.make_frames(args.batch, args.height, args.width, seed0=0))).cuda(0)
    engines = {}
    keep = []
    for dt in ("bf16", "fp16"):
        net, _ = workload.build_net(nref=1, seed=1, device=0, dtype=dt, height=args.height, width=args.width)
        keep.append(net)
        engines[dt] = net.engine

    def run_steps(eng, k):
        pending = []
        for i in range(k):
            if len(pending) >= 2:
                eng.pipeline_fetch(pending.pop(0))
            eng.pipeline_submit(x, i & 1, 4, True)
            pending.append(i & 1)
        for s in pending:
            eng.pipeline_fetch(s)

    for eng in engines.values():
        run_steps(eng, args.warmup)
    torch.cuda.synchronize()
    blocks = {dt: [] for dt in engines}
    for b in range(args.blocks):
        order = ("bf16", "fp16") if b % 2 == 0 else ("fp16", "bf16")
        for dt in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run_steps(engines[dt], args.steps)
            torch.cuda.synchronize()
            blocks[dt].append(args.batch * args.steps / (time.perf_counter() - t0))
    med = {dt: sorted(v)[(len(v) - 1) // 2] for dt, v in blocks.items()}
    print(json.dumps({"metric": "frames/s", "batch": args.batch, "height": args.height, "width": args.width, "steps": args.steps,
                      "bf16": med["bf16"], "fp16": med["fp16"], "fp16_over_bf16": med["fp16"] / med["bf16"],
                      "block_values": blocks}))


if __name__ == "__main__":
    main()
