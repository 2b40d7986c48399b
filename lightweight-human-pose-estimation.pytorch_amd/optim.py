"""The reference's optimiser for the stages (train.py:41-55 and :106), on the device.

``StageAdam(net)`` is ``torch.optim.Adam`` with train.py's parameter groups for every ``initial_stage.*`` /
``refinement_stages.*`` parameter of a drop-in net (fp32): conv weights x1 (initial) / x4 (refinement) with weight decay, conv
biases x2 / x8, refinement BatchNorm weights x1 and biases x2 without.  ``StageAdam(net, scope="cpm")`` also trains the cpm
(train.py:46-48): its conv weights x1 with weight decay, its biases x2 and its depthwise weights x1 without; the engine's
train scope is set on construction, ``val.train_step`` and the checkpoints below then cover the cpm.* keys too.
``StageAdam(net, scope="all")`` trains the backbone as well (train.py:42-45): stem and pointwise weights x1 with weight decay,
depthwise and BatchNorm weights x1 and BatchNorm biases x2 without, which is every group of the reference's optimiser.  The update and the refold / repack of the changed
layers into the forward's weight blob are HIP kernels behind ``lwp_stage_adam_step``: nothing travels through the host.

    opt = StageAdam(net, base_lr=4e-5, weight_decay=5e-4)
    for images, labels, masks in loader:
        losses = val.train_step(net, opt, images, labels, masks)
    sched = MultiStepLR(opt, [100, 200, 260], 0.333)      # train.py:60; sched.step() at the top of every epoch

``StageAdam(net, backward_precision="bf16")`` (or ``"fp16"``, with ``grad_scale`` a power of two) switches the engine's dense-conv
gradients to 16-bit MFMA operands (``Engine.set_backward_precision``); the parameters, the moments and the step stay fp32.

Out of scope: BatchNorm train mode (running statistics never move), no 16-bit forward in training, no 16-bit optimiser, no dynamic
loss scaling, multi-GPU gradient reduction and amsgrad.

Checkpoints come in two formats.  ``state_dict`` / ``load_state_dict`` have the package's own, keyed by state-dict name.
``torch_state_dict`` / ``load_torch_state_dict`` read and write what ``torch.optim.Adam.state_dict()`` gives for the optimiser of
train.py:41-55 (train.py:123 saves it, :69 loads it): index-based, the whole network numbered group by group (``torch_param_order``),
so a run started with the reference resumes here and the reverse.  ``MultiStepLR`` is train.py:60's schedule over a ``StageAdam``;
its state dict is interchangeable with ``torch.optim.lr_scheduler.MultiStepLR``'s.
"""
from collections import Counter, OrderedDict

import numpy as np


class StageAdam(object):
    def __init__(self, net, base_lr=4e-5, weight_decay=5e-4, betas=(0.9, 0.999), eps=1e-8, scope="stages", backward_precision=None,
                 grad_scale=None):
        self.net = net
        from . import _lib
        self.scope = _lib.train_scope_name(scope)
        if net.engine.train_scope != self.scope:   # (refused once the engine's optimiser has taken a step: the moments have the old layout)
            net.engine.set_train_scope(self.scope)
        if backward_precision is not None or grad_scale is not None:      # an argument left out keeps what the engine has
            name, scale = net.engine.backward_precision
            net.engine.set_backward_precision(name if backward_precision is None else backward_precision, scale if grad_scale is None else grad_scale)
        self.lr = float(base_lr)              # the base learning rate; the groups' multipliers are applied by the kernel
        self.weight_decay = float(weight_decay)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.accumulated = None               # flat gradient array of the iteration (val.train_step adds every batch to it)
        self.batch_index = 0                  # batches added since the last step
        self.steps = 0                        # steps taken through this object
        self.initial_lr = None                # the base rate a schedule started from (torch's group['initial_lr']); set by MultiStepLR

    @property
    def param_groups(self):
        """[(state-dict key, learning-rate multiplier, weight decay on)] under train.py:41-55."""
        return self.net.engine.adam_groups()

    def zero_grad(self):
        """Forgets the accumulated gradients (the next ``stage_backward`` of ``val.train_step`` overwrites)."""
        self.accumulated = None
        self.batch_index = 0

    def step(self, grads):
        """One Adam step from ``grads``: the dict ``Engine.stage_backward`` returned, or its flat array."""
        eng = self.net.engine
        flat = eng.flat_of(grads) if isinstance(grads, dict) else grads
        eng.adam_step(flat, self.lr, self.betas, self.eps, self.weight_decay)
        self.steps += 1

    # ---- checkpoints: {"step": int, "exp_avg": {key: tensor}, "exp_avg_sq": {key: tensor}}, float32 CPU tensors of the
    #      parameters' shapes keyed by state-dict name.  Not torch.optim.Adam's format.
    def state_dict(self):
        eng = self.net.engine
        st = eng.adam_state()
        out = OrderedDict(step=st["step"])
        for name in ("exp_avg", "exp_avg_sq"):
            out[name] = OrderedDict((k, v.cpu().clone()) for k, v in eng.grad_views(st[name]).items())
        return out

    def load_state_dict(self, state):
        import torch
        eng = self.net.engine
        spec, total = eng.grad_spec()
        flats = {}
        for name in ("exp_avg", "exp_avg_sq"):
            flat = torch.zeros(total, dtype=torch.float32)
            given = state[name]
            missing = [k for k, _, _ in spec if k not in given]
            unexpected = [k for k in given if k not in set(k for k, _, _ in spec)]
            if missing or unexpected:
                raise RuntimeError("Error(s) in loading %s: missing %s unexpected %s" % (name, missing, unexpected))
            for k, shape, off in spec:
                v = torch.as_tensor(np.asarray(given[k].detach().cpu() if hasattr(given[k], "detach") else given[k]), dtype=torch.float32)
                if tuple(v.shape) != tuple(shape):
                    raise RuntimeError("size mismatch for %s[%s]: %s vs %s" % (name, k, tuple(v.shape), tuple(shape)))
                flat[off:off + v.numel()] = v.reshape(-1)
            flats[name] = flat
        eng.load_adam_state(dict(step=int(state["step"]), exp_avg=flats["exp_avg"], exp_avg_sq=flats["exp_avg_sq"]))

    # ---- checkpoints in torch.optim.Adam's format (train.py:69, :123)
    def _torch_layout(self):
        eng = self.net.engine
        from . import _lib
        spec = [(k, shape) for k, shape, _ in _lib.param_spec(eng.nref, eng.C, eng.NH, eng.NP)]
        order = torch_param_order(spec)
        shapes = dict((k, tuple(shape)) for k, shape, _ in eng.grad_spec()[0])
        mine = dict((k, (mult, wd)) for k, mult, wd in self.param_groups)
        for g, keys in enumerate(order):       # the kernel's multipliers and the table below are two statements of train.py:41-55
            for k in keys:
                if k in mine and mine[k] != (TORCH_GROUPS[g][2], TORCH_GROUPS[g][3]):
                    raise RuntimeError("group %d: %s is %s in the engine's table" % (g, k, mine[k]))
        return order, shapes

    def torch_state_dict(self):
        """What ``torch.optim.Adam.state_dict()`` returns for train.py:41-55's optimiser in this state: thirteen ``param_groups``
        numbering every parameter of the network, and ``state`` for the parameters of the engine's train scope (empty before
        the first step)."""
        eng = self.net.engine
        order, shapes = self._torch_layout()
        st = eng.adam_state()
        moments = {}
        if st["step"] > 0:
            views = [eng.grad_views(st[name]) for name in ("exp_avg", "exp_avg_sq")]
            moments = dict((k, (views[0][k].cpu().clone(), views[1][k].cpu().clone())) for k in shapes)
        return pack_torch_state(order, dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                                            initial_lr=self.initial_lr), st["step"], moments)

    def load_torch_state_dict(self, sd):
        """The inverse: takes ``lr`` (group 0's), ``betas``, ``eps``, ``weight_decay`` and ``initial_lr`` from the groups and
        the step and moments of the train scope's parameters from ``state``.  ValueError, naming the group or the index, for
        anything that is not train.py:41-55's optimiser over this network (see ``unpack_torch_state``).  State of parameters
        outside the train scope is dropped; their number is printed."""
        import torch
        eng = self.net.engine
        order, shapes = self._torch_layout()
        hyper, step, moments, dropped = unpack_torch_state(sd, order, shapes)
        if dropped:
            print("[WARNING] Dropped the optimiser state of {} parameters outside train scope '{}'".format(dropped, self.scope))
        self.lr, self.betas, self.eps = hyper["lr"], hyper["betas"], hyper["eps"]
        self.weight_decay, self.initial_lr = hyper["weight_decay"], hyper["initial_lr"]
        if not moments:
            eng.load_adam_state(None)
            return
        spec, total = eng.grad_spec()
        flats = [torch.zeros(total, dtype=torch.float32), torch.zeros(total, dtype=torch.float32)]
        for k, shape, off in spec:
            for flat, v in zip(flats, moments[k]):
                flat[off:off + v.numel()] = v.reshape(-1)
        eng.load_adam_state(dict(step=step, exp_avg=flats[0], exp_avg_sq=flats[1]))


# ---------------------------------------------------------------------------------------------- torch's numbering, on the host
# train.py:41-55's thirteen groups: (state-dict prefix, kind, learning-rate multiplier, weight decay on)
TORCH_GROUPS = (("model.", "conv_w", 1, True), ("model.", "dw_w", 1, False), ("model.", "bn_w", 1, False), ("model.", "bn_b", 2, False),
                ("cpm.", "conv_w", 1, True), ("cpm.", "conv_b", 2, False), ("cpm.", "dw_w", 1, False),
                ("initial_stage.", "conv_w", 1, True), ("initial_stage.", "conv_b", 2, False),
                ("refinement_stages.", "conv_w", 4, True), ("refinement_stages.", "conv_b", 8, False),
                ("refinement_stages.", "bn_w", 1, False), ("refinement_stages.", "bn_b", 2, False))


def torch_param_order(state_spec):
    """The thirteen lists of state-dict keys in the order ``torch.optim.Adam`` numbers train.py:41-55's parameters: group by
    group, inside a group in module traversal order (not ``named_parameters()`` order over the network).  ``state_spec``:
    [(key, shape)] of the network's state dict in its own order (``_lib.param_spec``).  The group of a key follows from its
    name and shape as modules/get_parameters.py decides it from the module: a module with a ``running_mean`` is a BatchNorm2d,
    a 4-d weight with one input channel per group a depthwise conv, any other 4-d weight a dense conv.  Every parameter lands
    in exactly one group (ValueError otherwise); tests/golden/train_param_groups.json pins the result to the reference."""
    keys = set(k for k, _ in state_spec)
    groups = [[] for _ in TORCH_GROUPS]
    for key, shape in state_spec:
        module, _, name = key.rpartition(".")
        if name not in ("weight", "bias"):
            continue                                    # running_mean / running_var / num_batches_tracked: buffers
        if module + ".running_mean" in keys:
            kind = "bn_w" if name == "weight" else "bn_b"
        elif name == "bias":
            kind = "conv_b"
        else:
            kind = "dw_w" if len(shape) == 4 and shape[1] == 1 else "conv_w"
        hits = [g for g, (prefix, want, _, _) in enumerate(TORCH_GROUPS) if key.startswith(prefix) and kind == want]
        if len(hits) != 1:
            raise ValueError("%s %s is in %d of train.py's parameter groups" % (key, tuple(shape), len(hits)))
        groups[hits[0]].append(key)
    return groups


def _adam_constants():
    """The group entries the installed torch writes besides lr / betas / eps / weight_decay / params."""
    import torch
    g = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
    return dict((k, v) for k, v in g.items() if k not in ("lr", "betas", "eps", "weight_decay", "params"))


def pack_torch_state(order, hyper, step, moments):
    """``torch.optim.Adam.state_dict()`` of train.py:41-55's optimiser from plain values.  ``order``: ``torch_param_order``;
    ``hyper``: lr (the base rate), betas, eps, weight_decay, initial_lr (None without a schedule); ``moments``: key ->
    (exp_avg, exp_avg_sq) float32 CPU tensors for the parameters that have state ({} before the first step)."""
    import torch
    groups, state, first = [], {}, 0
    for (_, _, mult, wd), keys in zip(TORCH_GROUPS, order):
        g = dict(lr=mult * hyper["lr"], betas=tuple(hyper["betas"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"] if wd else 0)
        g.update(_adam_constants())
        if hyper.get("initial_lr") is not None:
            g["initial_lr"] = mult * hyper["initial_lr"]
        g["params"] = list(range(first, first + len(keys)))
        groups.append(g)
        for i, k in enumerate(keys, first):
            if k in moments:
                state[i] = dict(step=torch.tensor(float(step), dtype=torch.float32), exp_avg=moments[k][0], exp_avg_sq=moments[k][1])
        first += len(keys)
    return dict(state=state, param_groups=groups)


def unpack_torch_state(sd, order, shapes):
    """The inverse of ``pack_torch_state``: (hyper, step, moments, dropped).  ``shapes``: key -> shape of the parameters whose
    state is wanted (the train scope's); state of other parameters is counted in ``dropped``.  ValueError, naming the group or
    the index: not thirteen groups, a group of another length or numbering; amsgrad or maximize set; betas, eps or the non-zero
    weight_decay differing between groups, or a weight decay on a group the reference gives none; learning rates that are not
    {1, 2, 4, 8} x one base in the reference's pattern; a moment of the wrong shape; steps that are not all equal; a non-empty
    state that lacks a wanted parameter."""
    import torch
    groups = sd["param_groups"]
    if len(groups) != len(TORCH_GROUPS):
        raise ValueError("%d parameter groups, train.py's optimiser has %d" % (len(groups), len(TORCH_GROUPS)))
    g0, first, decay, key_of = groups[0], 0, None, {}
    base, initial = float(g0["lr"]), g0.get("initial_lr")
    for n, (g, (_, _, mult, wd), keys) in enumerate(zip(groups, TORCH_GROUPS, order)):
        if list(g["params"]) != list(range(first, first + len(keys))):
            raise ValueError("group %d: %d parameters numbered from %s, expected %d from %d"
                             % (n, len(g["params"]), g["params"][0] if len(g["params"]) else None, len(keys), first))
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("group %d: amsgrad / maximize is set" % n)
        if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
            raise ValueError("group %d: betas / eps differ from group 0's" % n)
        if g["lr"] != mult * base:
            raise ValueError("group %d: lr %r is not %d x the base rate %r" % (n, g["lr"], mult, base))
        if (initial is None) != (g.get("initial_lr") is None) or (initial is not None and g["initial_lr"] != mult * float(initial)):
            raise ValueError("group %d: initial_lr %r is not %d x group 0's %r" % (n, g.get("initial_lr"), mult, initial))
        if wd:
            if decay is not None and g["weight_decay"] != decay:
                raise ValueError("group %d: weight_decay %r differs from %r" % (n, g["weight_decay"], decay))
            decay = g["weight_decay"]
        elif g["weight_decay"] != 0:
            raise ValueError("group %d: weight_decay %r on a group the reference gives none" % (n, g["weight_decay"]))
        key_of.update(zip(g["params"], keys))
        first += len(keys)
    hyper = dict(lr=base, betas=(float(g0["betas"][0]), float(g0["betas"][1])), eps=float(g0["eps"]), weight_decay=float(decay),
                 initial_lr=None if initial is None else float(initial))
    step, moments, dropped = None, {}, 0
    for i, st in sd["state"].items():
        if i not in key_of:
            raise ValueError("state index %r: the optimiser has %d parameters" % (i, first))
        k = key_of[i]
        if k not in shapes:
            dropped += 1
            continue
        t = float(st["step"])
        if step is not None and t != step:
            raise ValueError("state index %d (%s): step %r, other parameters are at %r" % (i, k, t, step))
        step = t
        pair = []
        for name in ("exp_avg", "exp_avg_sq"):
            v = torch.as_tensor(st[name]).detach().to("cpu", torch.float32)
            if tuple(v.shape) != tuple(shapes[k]):
                raise ValueError("state index %d (%s): %s has shape %s, the parameter %s" % (i, k, name, tuple(v.shape), tuple(shapes[k])))
            pair.append(v)
        moments[k] = tuple(pair)
    if moments:
        lacking = [k for k in shapes if k not in moments]
        if lacking:
            index_of = dict((k, i) for i, k in key_of.items())
            raise ValueError("state index %d (%s): no state, though other parameters have one (%d lack it)"
                             % (index_of[lacking[0]], lacking[0], len(lacking)))
        if step != int(step):
            raise ValueError("state: step %r is not a whole number" % step)
    return hyper, int(step or 0), moments, dropped


class MultiStepLR(object):
    """train.py:60's ``optim.lr_scheduler.MultiStepLR(optimizer, milestones, gamma)`` over a ``StageAdam``: constructing it
    counts epoch 0, every ``step()`` one more, and at an epoch in ``milestones`` the CURRENT ``opt.lr`` is multiplied by
    ``gamma ** (times the epoch is listed)`` — torch's own arithmetic, so ``opt.lr`` follows torch's group 0 bit for bit; the
    other groups are powers of two times it.  As in torch, ``load_state_dict`` restores the counters and leaves ``opt.lr`` to
    the optimiser's own checkpoint.  The state dict has torch's entries and loads into torch's class, and torch's into this."""

    def __init__(self, opt, milestones, gamma=0.1):
        self.opt = opt
        if opt.initial_lr is None:
            opt.initial_lr = opt.lr
        self.milestones = Counter(milestones)
        self.gamma = gamma
        self.base_lrs = [g[2] * opt.initial_lr for g in TORCH_GROUPS]
        self.last_epoch = -1
        self._step_count = 0
        self.step()

    def step(self):
        self._step_count += 1
        self.last_epoch += 1
        if self.last_epoch in self.milestones:
            self.opt.lr = self.opt.lr * self.gamma ** self.milestones[self.last_epoch]
        self._last_lr = [g[2] * self.opt.lr for g in TORCH_GROUPS]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        return dict(milestones=Counter(self.milestones), gamma=self.gamma, base_lrs=list(self.base_lrs), last_epoch=self.last_epoch,
                    _step_count=self._step_count, _is_initial=False, _get_lr_called_within_step=False, _last_lr=list(self._last_lr))

    def load_state_dict(self, state):
        for name in ("milestones", "gamma", "base_lrs", "last_epoch", "_step_count", "_last_lr"):
            if name not in state:
                raise ValueError("scheduler state lacks %r" % name)
        self.milestones, self.gamma = Counter(state["milestones"]), state["gamma"]
        self.base_lrs, self._last_lr = list(state["base_lrs"]), list(state["_last_lr"])
        self.last_epoch, self._step_count = state["last_epoch"], state["_step_count"]
