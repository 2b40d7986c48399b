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
    opt.lr = opt.lr * 0.333            # MultiStepLR (train.py:60) is a line of Python

``StageAdam(net, backward_precision="bf16")`` (or ``"fp16"``, with ``grad_scale`` a power of two) switches the engine's dense-conv
gradients to 16-bit MFMA operands (``Engine.set_backward_precision``); the parameters, the moments and the step stay fp32.

Out of scope: BatchNorm train mode (running statistics never move), no 16-bit forward in training, no 16-bit optimiser, no dynamic
loss scaling, multi-GPU gradient reduction, amsgrad, and torch's optimiser checkpoints (``state_dict`` below has its own
format, keyed by state-dict name; torch's is index-based and numbers the whole network).
"""
from collections import OrderedDict

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
