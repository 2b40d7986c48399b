"""How much of a kernel's run time another stream's network kernels are running beside it, from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 300 --warmup 10
    python3 tools/stream_overlap.py DIR/*/*_kernel_trace.csv ["dwpw_kernel<16, 16"]

For every launch of the target kernel (default: the 512-output two-phase fused block) the share of its [start, end) interval
that is covered by the union of the NETWORK kernels (stem, depthwise, fused blocks, GEMM convs, stage heads) of the OTHER
streams; the figure printed is the sum of covered time over the sum of target time.  A stream is the trace's Stream_Id when it
has that column and is not constant, else its Queue_Id.  Also printed: launch-weighted average duration of the target and of
the dense 3x3 GEMM conv under the same load, and the number of network kernels running at a time (network kernel time / the
span they cover)."""
import bisect
import csv
import re
import sys

NETWORK = re.compile(r"lwp::(stem_kernel|dw_kernel|dwpw_|gemm_|heads_)")
DENSE3 = re.compile(r"gemm_ar_kernel<64, 4, \d, 0, 3>")


def read(path):
    rows = list(csv.DictReader(open(path, newline="")))
    key = "Queue_Id"
    if rows and "Stream_Id" in rows[0] and len({r["Stream_Id"] for r in rows if NETWORK.search(r["Kernel_Name"])}) > 1:
        key = "Stream_Id"
    out = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[key], r["Kernel_Name"]) for r in rows]
    return sorted(out), key


def main():
    path = sys.argv[1]
    target = sys.argv[2] if len(sys.argv) > 2 else "dwpw_kernel<16, 16"
    ks, key = read(path)
    net = [k for k in ks if NETWORK.search(k[3])]
    per = {}
    for s, e, q, _ in net:
        per.setdefault(q, []).append((s, e))
    starts = {q: [s for s, _ in v] for q, v in per.items()}
    longest = max(e - s for s, e, _, _ in net)
    tot = cov = n = 0
    for s, e, q, name in net:
        if target not in name:
            continue
        cl = []
        for q2, iv in per.items():
            if q2 == q:
                continue
            i = bisect.bisect_left(starts[q2], s - longest)
            while i < len(iv) and iv[i][0] < e:
                if iv[i][1] > s:
                    cl.append((max(iv[i][0], s), min(iv[i][1], e)))
                i += 1
        cl.sort()
        c, cur = 0, s
        for a, b in cl:
            if b > cur:
                c += b - max(a, cur)
                cur = b
        tot += e - s
        cov += c
        n += 1
    print("trace %s: %d kernels, %d network kernels on %d streams (%s)" % (path.split("/")[-1], len(ks), len(net), len(per), key))
    if n:
        print("%s: %d launches, average %.2f us, share of its time with another stream's network kernel beside it: %.3f" % (
            target, n, tot / n / 1e3, cov / tot))
    d3 = [e - s for s, e, _, name in net if DENSE3.search(name)]
    if d3:
        print("gemm_ar_kernel<64, 4, *, 0, 3>: %d launches, average %.2f us" % (len(d3), sum(d3) / len(d3) / 1e3))
    # network kernels running at a time: kernel time over the time at least one of them runs
    busy, cur = 0, None
    for s, e, _, _ in net:
        if cur is None or s > cur[1]:
            if cur:
                busy += cur[1] - cur[0]
            cur = [s, e]
        else:
            cur[1] = max(cur[1], e)
    busy += cur[1] - cur[0]
    print("network kernel time %.1f ms over %.1f ms with one running: %.2f at a time" % (
        sum(e - s for s, e, _, _ in net) / 1e6, busy / 1e6, sum(e - s for s, e, _, _ in net) / busy))


if __name__ == "__main__":
    main()
