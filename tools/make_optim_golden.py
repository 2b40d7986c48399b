"""Generates tests/golden/adam_groups.json: the parameter group (learning-rate multiplier, weight-decay flag) the reference's
optimiser gives every initial_stage.* / refinement_stages.* parameter.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_optim_golden.py

The reference's statements are executed, not restated: the ``optim.Adam([...], lr=base_lr, weight_decay=...)`` call is taken
out of train.py's syntax tree and evaluated on the reference's own PoseEstimationWithMobileNet with the reference's own
get_parameters_* predicates (modules/get_parameters.py); the groups torch builds from it are read back by parameter name.
The file holds names, multipliers and flags only."""
import ast
import json
import os
import sys

REF = os.environ.get("LWP_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "adam_groups.json")
# nref 0, 1, 2 with the default channels, and a custom skeleton (guide5 of tests/train_cases.py: 5 key-point types, 4 limbs)
CONFIGS = [(0, 128, 19, 38), (1, 128, 19, 38), (2, 128, 19, 38), (1, 128, 6, 8)]
BASE_LR = 0.25          # a power of two: every group's lr / BASE_LR is the exact multiplier


def adam_call():
    tree = ast.parse(open(os.path.join(REF, "train.py")).read())
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "Adam"]
    assert len(calls) == 1
    return compile(ast.Expression(calls[0]), "train.py", "eval")


def main():
    sys.path.insert(0, REF)
    from torch import optim
    from models.with_mobilenet import PoseEstimationWithMobileNet
    from modules import get_parameters as gp
    code = adam_call()
    out = {}
    for nref, C, NH, NP in CONFIGS:
        net = PoseEstimationWithMobileNet(nref, C, NH, NP)
        ns = dict(optim=optim, net=net, base_lr=BASE_LR, get_parameters_conv=gp.get_parameters_conv,
                  get_parameters_bn=gp.get_parameters_bn, get_parameters_conv_depthwise=gp.get_parameters_conv_depthwise)
        opt = eval(code, ns)
        name_of = {id(p): k for k, p in net.named_parameters()}
        rows, seen = [], set()
        for g in opt.param_groups:
            for p in g["params"]:
                k = name_of[id(p)]
                assert k not in seen, k
                seen.add(k)
                if k.startswith("initial_stage.") or k.startswith("refinement_stages."):
                    mult = g["lr"] / BASE_LR
                    assert mult == int(mult)
                    rows.append([k, int(mult), bool(g["weight_decay"] != 0)])
        order = {k: i for i, (k, _) in enumerate(net.named_parameters())}
        rows.sort(key=lambda r: order[r[0]])
        stage = [k for k, _ in net.named_parameters() if k.startswith("initial_stage.") or k.startswith("refinement_stages.")]
        assert [r[0] for r in rows] == stage, "a stage parameter is in no group"
        out["%d,%d,%d,%d" % (nref, C, NH, NP)] = rows
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(r) for r in out[k])) for k in sorted(out)) + "\n}\n")
    print(os.path.getsize(OUT), OUT)


if __name__ == "__main__":
    main()
