"""CPU: the float64 Adam restatement of tests/optim_cases.py against torch.optim.Adam with train.py:41-55's six stage groups,
lwp_stage_adam_group against the groups the reference's own optimiser builds (tests/golden/adam_groups.json), and the pinned
float64 fine-tuning loop of case d."""
import json
import os

import numpy as np
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth

import optim_cases as oc

from conftest import GOLDEN


def test_adam_ref_equals_torch_adam_float64_with_the_six_groups():
    """3 steps, weight decay on, within 1e-12 of the largest parameter change."""
    nref, C, NH, NP = 1, 32, 19, 38
    sd = synth.make_state_dict(nref, seed=3, num_channels=C, num_heatmaps=NH, num_pafs=NP)
    spec, total = _lib.stage_grad_spec(nref, C, NH, NP)
    base_lr = 1e-3
    rng = np.random.RandomState(4)
    params = {k: torch.nn.Parameter(sd[k].double().clone()) for k, _, _ in spec}
    by_group = {}
    for k, _, _ in spec:
        by_group.setdefault(oc.kind_of(k), []).append(k)
    assert sorted(by_group) == [0, 1, 2, 3, 4, 5]
    groups = []
    for kind, keys in sorted(by_group.items()):
        mult, wd = oc.GROUPS[kind]
        g = {"params": [params[k] for k in keys], "lr": base_lr * mult}
        if not wd:
            g["weight_decay"] = 0
        groups.append(g)
    opt = torch.optim.Adam(groups, lr=base_lr, betas=oc.BETAS, eps=oc.EPS, weight_decay=oc.WEIGHT_DECAY)
    p = {k: sd[k].double().numpy().copy() for k, _, _ in spec}
    start = {k: v.copy() for k, v in p.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    for t in range(1, 4):
        grads = {k: rng.standard_normal(p[k].shape) * 10.0 ** rng.randint(-6, 2) for k in p}
        for k in p:
            params[k].grad = torch.from_numpy(grads[k].copy())
            mult, wd = oc.group_of(k)
            p[k], m[k], v[k] = oc.adam_ref(p[k], grads[k], m[k], v[k], t, base_lr * mult, wd)
        opt.step()
    change = max(float(np.abs(p[k] - start[k]).max()) for k in p)
    worst = max(float(np.abs(p[k] - params[k].detach().numpy()).max()) for k in p)
    print("largest change %.3g, worst difference %.3g" % (change, worst))
    assert change > 0 and worst <= 1e-12 * change
    for k in p:
        st = opt.state[params[k]]
        assert np.abs(m[k] - st["exp_avg"].numpy()).max() <= 1e-12 * max(np.abs(m[k]).max(), 1e-300)
        assert np.abs(v[k] - st["exp_avg_sq"].numpy()).max() <= 1e-12 * max(np.abs(v[k]).max(), 1e-300)


def test_groups_match_the_reference_optimiser():
    with open(os.path.join(GOLDEN, "adam_groups.json")) as f:
        golden = json.load(f)
    assert len(golden) == 4
    for cfg, rows in golden.items():
        nref, C, NH, NP = (int(v) for v in cfg.split(","))
        got = _lib.stage_adam_groups(nref, C, NH, NP)
        assert [list(g) for g in got] == rows, cfg
        assert [oc.group_of(k) for k, _, _ in rows] == [(m, w) for _, m, w in rows], cfg
    assert set(nref for nref, _, _, _ in (tuple(int(v) for v in c.split(",")) for c in golden)) == {0, 1, 2}


def test_every_gradient_entry_falls_in_exactly_one_group():
    for nref, C, NH, NP in ((1, 128, 19, 38), (2, 32, 6, 8), (0, 32, 19, 38), (3, 64, 19, 38)):
        spec, total = _lib.stage_grad_spec(nref, C, NH, NP)
        groups = _lib.stage_adam_groups(nref, C, NH, NP)
        assert [k for k, _, _ in groups] == [k for k, _, _ in spec]          # one row per entry, in order
        for k, mult, wd in groups:
            kinds = [k.startswith("initial_stage.") and k.endswith(".weight"),
                     k.startswith("initial_stage.") and k.endswith(".bias"),
                     k.startswith("refinement_stages.") and not _is_bn(k) and k.endswith(".weight"),
                     k.startswith("refinement_stages.") and not _is_bn(k) and k.endswith(".bias"),
                     _is_bn(k) and k.endswith(".weight"),
                     _is_bn(k) and k.endswith(".bias")]
            assert sum(kinds) == 1, k
            assert (mult, wd) == [(1, True), (2, False), (4, True), (8, False), (1, False), (2, False)][kinds.index(True)], k
    L = _lib.lib()
    import ctypes as C_
    a, b = C_.c_int(), C_.c_int()
    assert L.lwp_stage_adam_group(1, 128, 19, 38, -1, C_.byref(a), C_.byref(b)) == _lib.LWP_ERR_ARG
    assert L.lwp_stage_adam_group(1, 128, 19, 38, len(_lib.stage_grad_spec(1)[0]), C_.byref(a), C_.byref(b)) == _lib.LWP_ERR_ARG


def _is_bn(key):
    """A BatchNorm parameter: its shape is (C,) and its module has running statistics in the state dict."""
    return key.rsplit(".", 1)[0] + ".running_mean" in _BN_KEYS


_BN_KEYS = set(synth.make_state_dict(3, seed=0, num_channels=32).keys())


def test_new_exports():
    for name in ("lwp_stage_adam_group", "lwp_stage_adam_step", "lwp_stage_params_get", "lwp_stage_adam_state_get",
                 "lwp_stage_adam_state_set", "lwp_stage_adam_reset", "lwp_time_stage_adam_step"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_pinned_float64_loop_of_case_d():
    losses = oc.float64_loop()
    assert len(losses) == oc.LOOP_STEPS + 1
    print("loss", losses[0], "->", losses[-1])
    assert abs(losses[0] - oc.LOOP_LOSS0) <= 1e-9 * oc.LOOP_LOSS0
    assert abs(losses[-1] - oc.LOOP_LOSS20) <= 1e-6 * oc.LOOP_LOSS0
    assert oc.LOOP_LOSS20 <= 0.5 * oc.LOOP_LOSS0                     # the chosen learning rate at least halves the loss
