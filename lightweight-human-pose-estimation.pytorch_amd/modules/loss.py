"""Drop-in for the reference's ``modules.loss`` (reference: modules/loss.py), computed by ``lwp_stage_losses``."""


def _channel_mask(mask):
    """The one (N, h, w) mask behind a per-channel mask tensor; the kernel broadcasts it and never reads a channel copy."""
    if mask.dim() == 3:
        return mask
    if mask.dim() != 4:
        raise ValueError("mask must be (N, C, h, w) or (N, h, w), got %s" % (tuple(mask.shape),))
    if mask.shape[1] > 1 and mask.stride(1) != 0 and not bool((mask == mask[:, :1]).all()):
        raise ValueError("the mask differs between channels: only one mask per frame, repeated over the channels "
                         "(as datasets/coco.py builds keypoint_mask and paf_mask), is supported")
    return mask[:, 0]


def l2_loss(input, target, mask, batch_size, engine=None):
    """``((input - target) * mask) ** 2 / 2 / batch_size`` summed over all elements, as a 0-d float64 cuda tensor, so
    ``loss.item()`` works as at train.py:96.  The terms and the sum are float64 (the reference's are float32) and the order
    of the sum is fixed.  There is NO ``.backward()``: the value comes from a HIP reduction outside autograd; gradients and
    the optimiser are out of scope.

    ``input``: (N, C, h, w) cuda tensor with C the engine's heat-map or PAF channel count; ``engine``: the ``Engine`` (or
    net) whose channel counts say which of the two it is, default the shared 19 / 38-channel engine of ``input``'s device.
    For all stages of a step in one launch use ``Engine.stage_losses`` / ``val.stage_losses``."""
    import torch
    from ..runtime import default_engine
    if not getattr(input, "is_cuda", False):
        raise RuntimeError("lwpose_amd has no CPU execution path")
    eng = default_engine(input.device.index) if engine is None else getattr(engine, "engine", engine)
    C = int(input.shape[1])
    if C == eng.NH:
        slot = 0
    elif C == eng.NP:
        slot = 1
    else:
        raise ValueError("input has %d channels; the engine's tensors have %d (heat-maps) or %d (PAFs): pass engine=" % (C, eng.NH, eng.NP))
    outs = [None] * (2 * (eng.nref + 1))
    outs[slot] = input
    losses = eng.stage_losses(outs, None if slot else target, target if slot else None, _channel_mask(mask), batch_size)
    return torch.tensor(losses[slot], dtype=torch.float64, device=input.device)
