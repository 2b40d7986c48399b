"""Drop-in for the reference's ``models.with_mobilenet.PoseEstimationWithMobileNet``
(reference: models/with_mobilenet.py:89-123), backed by the HIP engine.

Same constructor, ``state_dict`` keys/shapes, ``load_state_dict``, ``eval``/``cuda`` and call
convention: ``net(x)`` with x (N,3,H,W) float32 returns the list [heat0, paf0, heat1, paf1, ...]
of (N,{19,38},H/8,W/8) tensors on x's device.  There is no CPU execution path: a CPU tensor is
staged to the GPU by the library and the results are copied back.
"""
from collections import OrderedDict

import numpy as np

from .. import _lib, synth
from ..runtime import Engine


class PoseEstimationWithMobileNet(object):
    def __init__(self, num_refinement_stages=1, num_channels=128, num_heatmaps=19, num_pafs=38, dtype="fp32"):
        import torch
        self.num_refinement_stages = num_refinement_stages
        self.num_channels, self.num_heatmaps, self.num_pafs = num_channels, num_heatmaps, num_pafs
        self.dtype = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}[dtype]
        # parameters start from a deterministic random init (the reference starts from torch's default init)
        self._state = synth.make_state_dict(num_refinement_stages, seed=0, num_channels=num_channels,
                                            num_heatmaps=num_heatmaps, num_pafs=num_pafs)
        self._engine = None
        self._dirty = True
        self._seen_steps = 0           # Engine.stage_steps when self._state last agreed with the engine's stage parameters
        self._device_id = None
        self.training = False
        self._torch = torch

    # ---- nn.Module-like surface used by the reference's callers (demo.py:82-84,156-158; val.py:114,174-178)
    def _sync_from_engine(self):
        """After an optimiser step (Engine.adam_step, however it was reached) the engine holds the current stage parameters
        (and cpm / backbone parameters, where a train scope "cpm" / "all" has stepped, whatever the scope is now; the running
        statistics stay as loaded): copied back only when somebody asks."""
        eng = self._engine
        if eng is not None and eng.stage_steps != self._seen_steps:
            for k, v in eng.trained_params().items():
                self._state[k] = v.detach().cpu().to(self._state[k].dtype).reshape(self._state[k].shape).clone()
            self._seen_steps = eng.stage_steps

    def state_dict(self):
        self._sync_from_engine()
        return OrderedDict((k, v.clone()) for k, v in self._state.items())

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self._state if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._state]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict: missing %s unexpected %s" % (missing, unexpected))
        self._sync_from_engine()
        for k in self._state:
            if k in state_dict:
                v = state_dict[k]
                v = v.detach().cpu() if hasattr(v, "detach") else self._torch.as_tensor(np.asarray(v))
                if tuple(v.shape) != tuple(self._state[k].shape):
                    raise RuntimeError("size mismatch for %s: %s vs %s" % (k, tuple(v.shape), tuple(self._state[k].shape)))
                self._state[k] = v.to(self._state[k].dtype).clone()
        self._dirty = True

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("lwpose_amd has no training mode (no BatchNorm batch statistics): val.train_step / optim.StageAdam fine-tune the stages (in scope \"cpm\" the cpm too, in scope \"all\" the whole network) of the eval() network (BatchNorm at running statistics)")
        return self

    def cuda(self, device=None):
        idx = 0 if device is None else (device if isinstance(device, int) else self._torch.device(device).index or 0)
        self._ensure(idx)
        return self

    def to(self, device):
        d = self._torch.device(device)
        if d.type != "cuda":
            raise RuntimeError("lwpose_amd has no CPU execution path")
        return self.cuda(d.index or 0)

    def cpu(self):
        raise RuntimeError("lwpose_amd has no CPU execution path")

    @property
    def engine(self):
        self._ensure(self._device_id if self._device_id is not None else 0)
        return self._engine

    def _ensure(self, device_id):
        if self._engine is None or self._device_id != device_id:
            self._sync_from_engine()
            self._engine = Engine(device_id, self.num_refinement_stages, self.num_channels, self.num_heatmaps,
                                  self.num_pafs, self.dtype)
            self._device_id = device_id
            self._seen_steps = 0
            self._dirty = True
        if self._dirty:
            self._engine.load_state_dict(self._state)
            self._dirty = False

    def forward(self, x):
        dev = x.device.index if getattr(x, "is_cuda", False) else (self._device_id if self._device_id is not None else 0)
        self._ensure(dev)
        return self._engine.forward(x)

    __call__ = forward
