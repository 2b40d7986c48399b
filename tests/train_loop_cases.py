"""Shared by tests/test_train_loop_host.py and tests/test_gpu_train_loop.py: the fixtures of tools/make_train_loop_golden.py, a CPU
``torch.optim.Adam`` built the way train.py:41-55 builds it (parameters by key and shape, grouped by the fixture), the
synthetic MobileNet checkpoint of the ``load_from_mobilenet`` fixture, and a fake net / engine / dataset that let
``train.train`` run its loop control without a GPU."""
import json
import os

import numpy as np
import torch

from lwpose_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BASE_LR = 4e-5

# train.py:41-55: what each of the thirteen groups passes besides its parameters, as factors of base_lr (None: no 'lr' entry)
REF_GROUP_OPTIONS = [(None, None), (None, 0), (None, 0), (2, 0), (1, None), (2, 0), (None, 0), (1, None), (2, 0), (4, None), (8, 0),
                     (None, 0), (2, 0)]
MULTIPLIERS = [1, 1, 1, 2, 1, 2, 1, 1, 2, 4, 8, 1, 2]
NREF1_SIZES = [12, 11, 23, 23, 5, 2, 3, 7, 7, 19, 19, 10, 10]
NREF1_FIRST = [0, 12, 23, 46, 69, 74, 76, 79, 86, 93, 112, 131, 141]


def param_groups_fixture():
    with open(os.path.join(GOLDEN, "train_param_groups.json")) as f:
        return json.load(f)


def mobilenet_fixture():
    with open(os.path.join(GOLDEN, "load_from_mobilenet.json")) as f:
        return json.load(f)


def state_spec(nref, C=128, NH=19, NP=38):
    """[(key, shape)] of the network's state dict (the library's own table; no GPU)."""
    return [(k, tuple(shape)) for k, shape, _ in _lib.param_spec(nref, C, NH, NP)]


def torch_adam(nref, C=128, NH=19, NP=38, base_lr=BASE_LR, seed=0, values=None):
    """(optimiser, {key: Parameter}): CPU parameters by key and shape, grouped by the fixture, ``torch.optim.Adam`` with the
    reference's group options.  ``values``: key -> initial tensor (seeded random values otherwise)."""
    shapes = dict(state_spec(nref, C, NH, NP))
    g = torch.Generator().manual_seed(seed)
    params, groups = {}, []
    for keys, (mult, wd) in zip(param_groups_fixture()[str(nref)], REF_GROUP_OPTIONS):
        for k in keys:
            v = torch.randn(shapes[k], generator=g) * 0.05 if values is None else values[k].detach().clone().float().reshape(shapes[k])
            params[k] = torch.nn.Parameter(v)
        group = {"params": [params[k] for k in keys]}
        if mult is not None:
            group["lr"] = base_lr * mult
        if wd is not None:
            group["weight_decay"] = wd
        groups.append(group)
    return torch.optim.Adam(groups, lr=base_lr, weight_decay=5e-4), params


def seeded_steps(opt, params, steps, seed=1, only=None):
    """``steps`` optimiser steps with seeded gradients (for the keys in ``only``, or all); returns the gradients of each step."""
    g = torch.Generator().manual_seed(seed)
    taken = []
    for _ in range(steps):
        grads = {}
        for k, p in params.items():
            if only is None or k in only:
                p.grad = torch.randn(p.shape, generator=g) * 0.01
                grads[k] = p.grad.clone()
        opt.step()
        taken.append(grads)
    return taken


SCHEDULE_ENTRIES = ("last_epoch", "milestones", "gamma", "base_lrs", "_last_lr", "_step_count")


def schedules_equal(a, b):
    """Two schedule state dicts in the entries both classes must carry."""
    return all(a[k] == b[k] for k in SCHEDULE_ENTRIES)


def states_equal(a, b):
    """Two ``torch.optim.Adam.state_dict()``s: the same group dicts and the same tensors, bit for bit."""
    if a["param_groups"] != b["param_groups"] or sorted(a["state"]) != sorted(b["state"]):
        return False
    for i in a["state"]:
        sa, sb = a["state"][i], b["state"][i]
        if sorted(sa) != sorted(sb):
            return False
        for name in sa:
            if sa[name].dtype != sb[name].dtype or sa[name].shape != sb[name].shape or not torch.equal(sa[name], sb[name]):
                return False
    return True


# ------------------------------------------------------------------------------------------------ load_from_mobilenet
def mobilenet_source(fix):
    """The fixture's synthetic checkpoint: every tensor filled with 2, as tools/make_train_loop_golden.py made it."""
    return {"state_dict": {k: torch.full(tuple(shape), 2.0) for k, shape in fix["source"]}}


class DictNet(object):
    """state_dict / load_state_dict of a net whose values are all 1, on the host."""

    def __init__(self, nref):
        self.state = {k: torch.ones(shape) for k, shape in state_spec(nref)}

    def state_dict(self):
        return dict(self.state)

    def load_state_dict(self, sd):
        assert list(sd) == list(self.state)
        self.state = dict(sd)


# ------------------------------------------------------------------------------------------------ the loop with a fake engine
class FakeEngine(object):
    """What ``optim.StageAdam``, ``optim.MultiStepLR`` and ``train.train`` ask of an engine, on the host.  The layout tables are
    the library's own; the "kernels" count: ``adam_step`` adds the gradient to exp_avg and 1 to the step."""

    def __init__(self, nref, C=32, calls=None):
        self.nref, self.C, self.NH, self.NP = nref, C, 19, 38
        self.train_scope, self.backward_precision, self.device_id, self.stage_steps = "stages", ("fp32", 1.0), 0, 0
        self.calls = [] if calls is None else calls
        self.log, self.adds = [0.0] * (2 * (nref + 1)), 0
        self._reset()

    def _reset(self):
        total = self.grad_spec()[1]
        self.m, self.v, self.t = torch.zeros(total), torch.zeros(total), 0

    def set_train_scope(self, scope):
        self.train_scope = _lib.train_scope_name(scope)
        self._reset()

    def set_backward_precision(self, name, scale):
        self.backward_precision = (name, scale)

    def grad_spec(self):
        return _lib.train_grad_spec(self.train_scope, self.nref, self.C, self.NH, self.NP)

    def grad_views(self, flat):
        return dict((k, flat[off:off + int(np.prod(shape))].view(shape)) for k, shape, off in self.grad_spec()[0])

    def adam_groups(self):
        return _lib.train_adam_groups(self.train_scope, self.nref, self.C, self.NH, self.NP)

    def adam_step(self, flat, lr, betas, eps, weight_decay):
        self.calls.append(("adam", lr))
        self.m, self.t = self.m + flat, self.t + 1
        self.v = self.v + flat * flat
        self.stage_steps += 1

    def adam_state(self):
        return dict(step=self.t, exp_avg=self.m.clone(), exp_avg_sq=self.v.clone())

    def load_adam_state(self, state):
        if state is None:
            self._reset()
        else:
            self.m, self.v, self.t = state["exp_avg"].clone(), state["exp_avg_sq"].clone(), int(state["step"])

    def read_loss_log(self, reset=True):
        out = (list(self.log), self.adds)
        self.calls.append(("read", reset, out[1]))
        if reset:
            self.log, self.adds = [0.0] * len(self.log), 0
        return out


class FakeNet(object):
    def __init__(self, nref, calls, C=32):
        self.engine = FakeEngine(nref, C, calls=calls)
        self.weights = {"model.0.0.weight": torch.zeros(2, 3)}

    def cuda(self, device=None):
        return self

    def state_dict(self):
        return dict(self.weights)

    def load_state_dict(self, sd):
        self.weights = dict(sd)

    def train(self, mode=True):
        raise AssertionError("train() must never call net.train")


class FakeDataset(object):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def samples(self, indices):
        return list(indices)


def fake_loss(call, i):
    """Loss i of the call-th train step (counted from 1) of a fake run."""
    return call * (i + 1) / 8.0


def patch_train(monkeypatch, train_mod, n_samples, calls):
    """Replaces what ``train.train`` would run on the GPU; ``calls`` receives ("step", batch size, batch index seen), ("adam", lr),
    ("read", reset, adds), ("val", output name) in the order they happen."""
    steps = [0]

    def step(net, opt, samples, augment, batches_per_iter=1, sigma=7, paf_thickness=1, log=False):
        assert log is True
        eng = net.engine
        steps[0] += 1
        calls.append(("step", len(samples), opt.batch_index))
        if opt.batch_index == 0:
            opt.zero_grad()
        flat = torch.full((eng.grad_spec()[1],), 1.0 / batches_per_iter)
        opt.accumulated = flat if opt.accumulated is None else opt.accumulated + flat
        for i in range(len(eng.log)):
            eng.log[i] += fake_loss(steps[0], i) / batches_per_iter
        eng.adds += 1
        opt.batch_index += 1
        if opt.batch_index >= batches_per_iter:
            opt.step(opt.accumulated)
            opt.batch_index = 0

    def evaluate(labels, output_name, samples, net, store=False):
        assert store is True
        calls.append(("val", output_name))

    monkeypatch.setattr(train_mod, "PoseEstimationWithMobileNet", lambda nref: FakeNet(nref, calls))
    monkeypatch.setattr(train_mod, "CocoTrainDataset", lambda labels, folder, net, fallback, entropy: FakeDataset(n_samples))
    monkeypatch.setattr(train_mod, "CocoValDataset", lambda labels, folder, net, fallback, entropy: None)
    monkeypatch.setattr(train_mod, "DeviceAugment", lambda transforms, stride, rng: None)
    monkeypatch.setattr(train_mod, "augmented_train_step", step)
    monkeypatch.setattr(train_mod, "evaluate", evaluate)
