"""Generates tests/golden/train_param_groups.json and tests/golden/load_from_mobilenet.json.

Run only where the reference checkout exists (never on the GPU machines):

    python tools/make_train_loop_golden.py

train_param_groups.json: for num_refinement_stages 0, 1 and 3 the thirteen lists of state-dict keys of the reference's
optimiser, each in the order torch numbers its parameters (``torch.optim.Adam.state_dict()`` counts group by group).  As in
tools/make_optim_golden.py the reference's statements are executed, not restated: the ``optim.Adam([...])`` call is taken out
of train.py's syntax tree and evaluated on the reference's own network with the reference's own get_parameters_* predicates.

load_from_mobilenet.json: the reference's ``modules.load_state.load_from_mobilenet`` run on its own network against a synthetic
checkpoint (``module.model.*`` keys, a few keys outside the backbone, one tensor of a wrong shape, one key left out): the lines
it printed and the keys whose tensor it took from the checkpoint.  The checkpoint is described by key and shape; the test
rebuilds it.  Both files hold names, shapes and printed lines only, no tensors."""
import ast
import contextlib
import io
import json
import os
import sys

REF = os.environ.get("LWP_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NREFS = (0, 1, 3)
MISSING = "model.3.1.weight"                  # left out of the synthetic checkpoint
WRONG_SHAPE = "model.5.3.weight"              # present with one output channel too many
OUTSIDE = ("cpm.align.0.weight", "cpm.align.0.bias")      # keys without 'model' are looked up as they are


def adam_call():
    tree = ast.parse(open(os.path.join(REF, "train.py")).read())
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "Adam"]
    assert len(calls) == 1
    return compile(ast.Expression(calls[0]), "train.py", "eval")


def param_groups(PoseEstimationWithMobileNet, gp, optim):
    code = adam_call()
    out = {}
    for nref in NREFS:
        net = PoseEstimationWithMobileNet(nref)
        ns = dict(optim=optim, net=net, base_lr=0.25, get_parameters_conv=gp.get_parameters_conv,
                  get_parameters_bn=gp.get_parameters_bn, get_parameters_conv_depthwise=gp.get_parameters_conv_depthwise)
        opt = eval(code, ns)
        name_of = {id(p): k for k, p in net.named_parameters()}
        groups = [[name_of[id(p)] for p in g["params"]] for g in opt.param_groups]
        flat = [k for g in groups for k in g]
        assert len(flat) == len(set(flat)) and set(flat) == set(name_of.values()), "a parameter is in no group, or in two"
        # torch's own numbering, read back from the optimiser's state dict
        numbered = [g["params"] for g in opt.state_dict()["param_groups"]]
        assert [i for g in numbered for i in g] == list(range(len(flat)))
        assert [len(g) for g in numbered] == [len(g) for g in groups]
        out[str(nref)] = groups
    return out


def mobilenet_case(PoseEstimationWithMobileNet, load_from_mobilenet, torch):
    net = PoseEstimationWithMobileNet(1)
    target = net.state_dict()
    source = {}
    for k, v in target.items():
        if k == MISSING or not (k.startswith("model.") or k in OUTSIDE):
            continue
        shape = list(v.shape)
        if k == WRONG_SHAPE:
            shape[0] += 1
        source[k.replace("model", "module.model")] = torch.full(shape, 2.0, dtype=v.dtype)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        load_from_mobilenet(net, {"state_dict": source})
    after = net.state_dict()
    taken = [k for k, v in after.items() if v.numel() and bool((v == 2).all())]
    return dict(num_refinement_stages=1, missing=MISSING, wrong_shape=WRONG_SHAPE,
                source=[[k, list(v.shape)] for k, v in source.items()], printed=buf.getvalue().splitlines(), taken=taken)


def main():
    sys.path.insert(0, REF)
    import torch
    from torch import optim
    from models.with_mobilenet import PoseEstimationWithMobileNet
    from modules import get_parameters as gp
    from modules.load_state import load_from_mobilenet
    groups = param_groups(PoseEstimationWithMobileNet, gp, optim)
    path = os.path.join(GOLDEN, "train_param_groups.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('"%s": [\n%s\n]' % (k, ",\n".join(json.dumps(g) for g in groups[k])) for k in sorted(groups)) + "\n}\n")
    print(os.path.getsize(path), path)
    case = mobilenet_case(PoseEstimationWithMobileNet, load_from_mobilenet, torch)
    path = os.path.join(GOLDEN, "load_from_mobilenet.json")
    with open(path, "w") as f:
        json.dump(case, f, indent=0)
        f.write("\n")
    print(os.path.getsize(path), path)


if __name__ == "__main__":
    main()
