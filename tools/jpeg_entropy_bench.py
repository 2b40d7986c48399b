"""The device entropy decoder of the JPEG reader against the host decode of the same commit.

    python tools/jpeg_entropy_bench.py [--batch 80] [--iters 10] [--out profiles/train/jpeg_entropy_bench.json]

Workload: tools/jpeg_bench.py's (``batch`` files of 480 x 640, 4:2:0, quality 90, textured synthetic content made with Pillow;
without Pillow the tool records that and quotes no figure).  Records
  - the host pre-pass (lwp_debug_jpeg_scan through ctypes: un-stuffing, segments, tables) per batch on 1 and on 16 threads, and
    the host Huffman decode it replaces (lwp_debug_jpeg_blocks) the same way;
  - the bytes of the one upload in device mode (file bytes, flattened tables, records) next to host mode's coefficients;
  - the entropy kernels' device time (memset and the four kernels) by HIP events around back-to-back runs
    (lwp_time_jpeg_entropy_batch), three windows, the median, at subseq_bytes 32 / 64 / 128 / 256, with the sync rounds taken
    inside a workgroup and across workgroups;
  - the whole decode_jpeg_batch call in device mode against host mode, alternating windows;
  - the fixed cost of the status wait: a copy of the N + 2 status words to the host and the synchronise, on an idle stream
    (in a call the wait also lasts until the entropy kernels have finished).
No ratio is fixed in advance; the default mode stays the host whatever the figures."""
import argparse
import io
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import _lib  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402
from jpeg_bench import textured, wall_ms  # noqa: E402

import ctypes as C  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "jpeg_entropy_bench.json"))
    a = ap.parse_args()
    N, H, W = a.batch, 480, 640
    out = {"workload": "batch %d, %dx%d, 4:2:0, quality 90, textured synthetic content" % (N, H, W), "iters": a.iters}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        out["pillow"] = "absent: no input files, no figure"
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    files = []
    for n in range(N):
        buf = io.BytesIO()
        Image.fromarray(textured(H, W, n)).save(buf, "JPEG", quality=90, subsampling=2)
        files.append(buf.getvalue())
    out["file_bytes"] = int(sum(len(f) for f in files))
    L = _lib.lib()
    heads = [Engine.jpeg_info(f) for f in files]
    blocks = sum(h["total_blocks"] for h in heads)
    longest = max(len(f) for f in files)
    scratch = {}

    def buffers():
        key = threading.get_ident()
        if key not in scratch:
            scratch[key] = (np.empty(longest + 8, dtype=np.uint8), np.empty(4, dtype=np.uint32), np.empty(6 * 1488, dtype=np.uint8),
                            np.empty(256, dtype=np.uint16), np.empty(heads[0]["total_blocks"] * 64, dtype=np.int16))
        return scratch[key]

    def prepass_one(f):
        raw, segs, tables, qt, _ = buffers()
        nb, ns, status = C.c_size_t(), C.c_size_t(), C.c_int()
        rc = L.lwp_debug_jpeg_scan(f, len(f), raw.ctypes.data, raw.size, C.byref(nb), segs.ctypes.data, 1, C.byref(ns), tables.ctypes.data,
                                   qt.ctypes.data, C.byref(status))
        assert rc == 0 and status.value == 0

    def host_one(f):
        _, _, _, qt, coef = buffers()
        assert L.lwp_debug_jpeg_blocks(f, len(f), coef.ctypes.data, coef.size, qt.ctypes.data) == 0

    def batch_ms(fn, threads):
        t0 = time.perf_counter()
        if threads == 1:
            for f in files:
                fn(f)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(fn, files))
        return (time.perf_counter() - t0) * 1e3
    for key, fn in (("pre_pass", prepass_one), ("host_entropy", host_one)):
        batch_ms(fn, 1)
        for threads in (1, 16):
            runs = [batch_ms(fn, threads) for _ in range(3)]
            out["%s_ms_per_batch_%d_thread%s_runs" % (key, threads, "s" if threads > 1 else "")] = runs
            out["%s_ms_per_batch_%d_thread%s" % (key, threads, "s" if threads > 1 else "")] = float(np.median(runs))
    out["upload_bytes_device_mode"] = int(sum((len(f) + 3) // 4 * 4 + 8 for f in files) + N * (6 * 1488 + 512 + 64 + 24 + 8) + 4096)
    out["upload_bytes_host_mode"] = int(blocks * 128 + N * 512 + 4096)

    eng = Engine(0, nref=1, num_channels=32)           # the decode needs no weights
    k = 2 * a.iters
    sweep = {}
    for subseq in (32, 64, 128, 256):
        eng.debug_jpeg_entropy(files, subseq, time_iters=2)
        runs = [eng.debug_jpeg_entropy(files, subseq, time_iters=k) for _ in range(3)]
        sweep[str(subseq)] = {"entropy_kernels_ms_runs": [r[0] / k for r in runs], "entropy_kernels_ms": float(np.median([r[0] / k for r in runs])),
                              "sync_rounds_in_a_workgroup": runs[0][1], "sync_rounds_across_workgroups": runs[0][2],
                              "subsequences": int(sum(-(-len(f) // subseq) for f in files))}
    out["kernel_runs_timed"] = k
    out["subseq_bytes_sweep"] = sweep

    host_mode, device_mode = [], []
    for _ in range(3):
        host_mode.append(wall_ms(lambda: eng.decode_jpeg_batch(files, entropy="host"), a.iters))
        device_mode.append(wall_ms(lambda: eng.decode_jpeg_batch(files, entropy="device"), a.iters))
    out["decode_jpeg_batch_host_mode_ms_runs"], out["decode_jpeg_batch_device_mode_ms_runs"] = host_mode, device_mode
    out["decode_jpeg_batch_host_mode_ms"] = float(np.median(host_mode))
    out["decode_jpeg_batch_device_mode_ms"] = float(np.median(device_mode))
    out["device_mode_subseq_bytes"] = 128
    words = torch.zeros(N + 2, dtype=torch.int32, device="cuda")
    pinned = torch.empty(N + 2, dtype=torch.int32).pin_memory()
    out["status_wait_idle_stream_ms"] = float(np.median([wall_ms(lambda: (pinned.copy_(words, non_blocking=True), torch.cuda.synchronize()), a.iters)
                                                         for _ in range(3)]))
    got = eng.decode_jpeg_batch(files, entropy="device")
    want = eng.decode_jpeg_batch(files, entropy="host")
    out["bytes_differing_between_the_modes"] = int(sum(int((g != w).sum()) for g, w in zip(got, want)))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
