"""Do two layers of two engine streams share the chip?  No profiler (a kernel trace nearly serialises the streams).

    python3 tools/corun_layers.py [layer_a] [layer_b] [iters]        default: model.8.pw (fused 512 -> 512) beside cpm.conv (dense 3x3)

Two engines (own streams) each repeat ONE layer at the benchmark's frame (1 x 368 x 656) with HIP events around the run
(lwp_debug_time_layer): first each alone, then both at once from two threads.  us per launch alone and together; if the two
kernels exclude each other the together figures are about the sum of the alone ones for both, if they run side by side they
stay near the alone ones.  LWP_DWPW_LEAN etc. are read at engine creation, so one library gives both forms."""
import os
import sys
import threading
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lwpose_amd  # noqa: F401,E402
from lwpose_amd import _lib, synth  # noqa: E402
from lwpose_amd.runtime import Engine  # noqa: E402

la = sys.argv[1] if len(sys.argv) > 1 else "model.8.pw"
lb = sys.argv[2] if len(sys.argv) > 2 else "cpm.conv"
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 4000
sd = synth.make_state_dict(1, seed=1)
engs = []
for _ in range(2):
    e = Engine(0, nref=1, dtype=_lib.F32)
    e.load_state_dict(sd)
    engs.append(e)
idx = {l["name"]: l["index"] for l in engs[0].layers()}
H, W = 368, 656


def t(e, name, n):
    return e.time_layer(idx[name], 1, H, W, n) * 1e3


alone_a, alone_b = t(engs[0], la, iters), t(engs[1], lb, iters)
# together: b runs long enough to cover a from start to end, then a long enough to cover b
res = {}


def th(key, e, name, n):
    res[key] = t(e, name, n)


def both(na, nb):
    ts = [threading.Thread(target=th, args=("a", engs[0], la, na)), threading.Thread(target=th, args=("b", engs[1], lb, nb))]
    ts[1 if nb > na else 0].start()
    ts[0 if nb > na else 1].start()
    for x in ts:
        x.join()
    return res["a"], res["b"]


a_cov, _ = both(iters, int(iters * 3 * max(1.0, alone_a / alone_b)))
_, b_cov = both(int(iters * 3 * max(1.0, alone_b / alone_a)), iters)
print("LWP_DWPW_LEAN=%s  %s alone %.2f us, beside %s %.2f us;  %s alone %.2f us, beside %s %.2f us  (sum of alone %.2f)" % (
    os.environ.get("LWP_DWPW_LEAN", "unset"), la, alone_a, lb, a_cov, lb, alone_b, la, b_cov, alone_a + alone_b))
