"""JPEG files to BGR pixels on the device: Engine.decode_jpeg_batch against the route a user has without it (Pillow on the host,
channel reverse, upload).

    python tools/jpeg_bench.py [--batch 80] [--iters 10] [--out profiles/train/jpeg_bench.json]

Workload: ``batch`` files of 480 x 640, 4:2:0, quality 90, textured synthetic content (made with Pillow; without Pillow the tool
records that and quotes no figure).  Records, separately,
  - the host half (marker parse + Huffman decode, lwp_debug_jpeg_blocks through ctypes) per batch on one thread and on a pool
    of 16 threads (the call holds no lock and ctypes drops the GIL);
  - the bytes of the one upload (coefficients, tables, descriptors) and the time of a pinned copy of that size;
  - stage A (inverse DCT) and stage B (up-sample, colour, store) device time: HIP events around back-to-back launches
    (lwp_time_jpeg_decode_batch), three windows, the median; the bytes each moves against the 8 TB/s HBM figure, untuned;
  - the whole decode_jpeg_batch call (header pass, host decode on the call's own threads, 16 at the most, staging, upload,
    both kernels, synchronise);
  - the baseline on the same commit, alternating with it: Pillow decode (1 and 16 threads), channel reverse, upload.
No ratio is fixed in advance.  The upload is the int16 coefficients, about twice the pixels' bytes at 4:2:0: the call takes the
inverse DCT, the up-sampling and the colour conversion off the host, not the PCIe bytes."""
import argparse
import ctypes
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lwpose_amd  # noqa: E402,F401
from lwpose_amd import _lib  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

HBM_BYTES_PER_S = 8e12


def textured(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        a, b, p = g.uniform(0.02, 0.3, 3)
        img[:, :, c] = 128 + 70 * np.sin(a * x + 5 * p) * np.cos(b * y + c) + 30 * np.sin(0.9 * x + 1.3 * y + c)
    img += g.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def wall_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train", "jpeg_bench.json"))
    a = ap.parse_args()
    N, H, W = a.batch, 480, 640
    out = {"workload": "batch %d, %dx%d, 4:2:0, quality 90, textured synthetic content" % (N, H, W), "iters": a.iters}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
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
    out["mean_file_bytes"] = float(np.mean([len(f) for f in files]))
    L = _lib.lib()
    heads = [Engine.jpeg_info(f) for f in files]
    blocks = sum(h["total_blocks"] for h in heads)

    # ---- host half alone
    def host_one(f, scratch={}):
        import threading
        key = threading.get_ident()
        if key not in scratch:
            scratch[key] = (np.empty(heads[0]["total_blocks"] * 64, dtype=np.int16), np.empty(256, dtype=np.uint16))
        coef, qt = scratch[key]
        assert L.lwp_debug_jpeg_blocks(f, len(f), coef.ctypes.data, coef.size, qt.ctypes.data) == 0

    def host_ms(threads):
        t0 = time.perf_counter()
        if threads == 1:
            for f in files:
                host_one(f)
        else:
            with ThreadPoolExecutor(threads) as ex:
                list(ex.map(host_one, files))
        return (time.perf_counter() - t0) * 1e3
    host_ms(1)
    out["host_entropy_ms_per_batch_1_thread_runs"] = [host_ms(1) for _ in range(3)]
    out["host_entropy_ms_per_batch_16_threads_runs"] = [host_ms(16) for _ in range(3)]
    out["host_entropy_ms_per_batch_1_thread"] = float(np.median(out["host_entropy_ms_per_batch_1_thread_runs"]))
    out["host_entropy_ms_per_batch_16_threads"] = float(np.median(out["host_entropy_ms_per_batch_16_threads_runs"]))

    # ---- the upload
    upload = blocks * 128 + N * 512 + 4096
    out["upload_bytes"] = int(upload)
    out["pixel_bytes"] = N * H * W * 3
    pinned = torch.empty(upload, dtype=torch.uint8).pin_memory()
    dev = torch.empty(upload, dtype=torch.uint8, device="cuda")
    out["pinned_copy_of_upload_size_ms"] = float(np.median([wall_ms(lambda: dev.copy_(pinned, non_blocking=True), a.iters) for _ in range(3)]))

    # ---- the kernels
    eng = Engine(0, nref=1, num_channels=32)           # the decode needs no weights
    eng.decode_jpeg_batch(files, time_iters=2)
    k = 10 * a.iters
    runs = [eng.decode_jpeg_batch(files, time_iters=k) for _ in range(3)]
    out["kernel_launches_timed"] = k
    out["stage_a_ms_runs"], out["stage_b_ms_runs"] = [r[0] / k for r in runs], [r[1] / k for r in runs]
    out["stage_a_ms"], out["stage_b_ms"] = float(np.median(out["stage_a_ms_runs"])), float(np.median(out["stage_b_ms_runs"]))
    out["stage_a_bytes"] = int(blocks * (128 + 64))
    out["stage_b_bytes"] = int(blocks * 64 + N * H * W * 3)
    for s in ("a", "b"):
        out["stage_%s_fraction_of_8TBs_untuned" % s] = out["stage_%s_bytes" % s] / (out["stage_%s_ms" % s] * 1e-3) / HBM_BYTES_PER_S

    # ---- whole calls, alternating with the baseline
    def pillow_one(f):
        return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(f)))[:, :, ::-1])

    def baseline(threads):
        if threads == 1:
            arrays = [pillow_one(f) for f in files]
        else:
            with ThreadPoolExecutor(threads) as ex:
                arrays = list(ex.map(pillow_one, files))
        return torch.from_numpy(np.stack(arrays)).cuda()
    ours, base1, base16 = [], [], []
    for _ in range(3):
        ours.append(wall_ms(lambda: eng.decode_jpeg_batch(files), a.iters))
        base1.append(wall_ms(lambda: baseline(1), a.iters))
        base16.append(wall_ms(lambda: baseline(16), a.iters))
    out["decode_jpeg_batch_ms_runs"], out["pillow_1_thread_ms_runs"], out["pillow_16_threads_ms_runs"] = ours, base1, base16
    out["decode_jpeg_batch_ms"] = float(np.median(ours))
    out["pillow_1_thread_reverse_upload_ms"] = float(np.median(base1))
    out["pillow_16_threads_reverse_upload_ms"] = float(np.median(base16))
    # what the call spends besides the entropy decode and the kernels: header pass, thread start, descriptors, upload, synchronise
    out["call_minus_host_16_threads_and_kernels_ms"] = (out["decode_jpeg_batch_ms"] - out["host_entropy_ms_per_batch_16_threads"] -
                                                        out["stage_a_ms"] - out["stage_b_ms"])
    got = eng.decode_jpeg_batch(files)
    want = baseline(1)
    out["bytes_differing_from_pillow"] = int(sum(int((g != w).sum()) for g, w in zip(got, want)))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
