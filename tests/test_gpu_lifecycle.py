"""GPU: a handle gives back everything it took.

Device memory, pinned memory, events and streams of the library are held by the owner types of csrc/lwp_owners.h, which
count what is alive (lwp_debug_live_resources).  An engine is driven through every entry point that takes a resource, at
shape A, the larger shape B and A again, and the four counters are compared with their reading before the engine existed
(other fixtures of the process may hold handles: nothing here is compared with zero).

Order of the calls: tracking mode 2 and overlay mode 2 are set once, in front of the three passes, and lwp_set_capacity runs
behind them.  Each of the three frees every workspace by contract, so inside the passes it would make the byte counts
depend on the last shape and the grow-only assertion (b) meaningless.  Results are not re-checked: the other tests do that."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, synth
from lwpose_amd.runtime import Engine

pytestmark = pytest.mark.gpu

SHAPE_A, SHAPE_B = (1, 64, 96), (3, 91, 149)         # B is larger in N, H and W: every grow-only buffer grows once


def live():
    out = (C.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)                  # device bytes, pinned bytes, events, streams


def quiet(fn, *args, **kw):
    """Random weights may overflow a capacity: the call has still taken (and kept) its buffers."""
    try:
        return fn(*args, **kw)
    except _lib.CapacityError:
        return None


def one_pass(eng, shape, fp32):
    N, H, W = shape
    rs = np.random.RandomState(N * 1000 + H)
    x = rs.uniform(-0.5, 0.5, size=(N, 3, H, W)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    frames = synth.make_frames(N, H, W, seed0=H)
    outs = eng.forward(x)                              # host in, host out: input and output staging
    quiet(eng.infer_poses, x)
    eng.infer_poses_async(xd)
    quiet(eng.fetch_poses)
    for slot in (0, 1):
        eng.pipeline_submit_u8(frames, slot, H)        # host frames: pinned upload, the slot's own frame copy, overlay buffers
    for slot in (0, 1):
        quiet(eng.pipeline_fetch, slot)
        assert eng.pipeline_overlay(slot).shape == (N, H, W, 3)
    heat = outs[-2]
    for ratio in (1.0, 0.5):
        xs, pad = eng.preprocess_scaled_u8(frames, ratio, H, 8)
        maps = eng.forward(xs)[-2].cpu().numpy()
        accum = np.zeros((N, H, W, maps.shape[1]), np.float32)
        eng.multiscale_accumulate(accum, maps, 8, pad, 2, init=ratio == 1.0)
    eng.upsample(heat, 4)
    if not fp32:
        return
    touts = eng.train_forward(xd)
    hs, ws = int(touts[0].shape[2]), int(touts[0].shape[3])
    kpts = np.zeros((N, 2, 18, 3), np.float64)
    kpts[..., 0] = rs.uniform(0, ws * 8, size=(N, 2, 18))
    kpts[..., 1] = rs.uniform(0, hs * 8, size=(N, 2, 18))
    kmaps, pmaps = eng.train_targets(kpts, np.full(N, 2), (hs * 8, ws * 8))
    mask = eng.mask_downsample(np.ones((N, hs * 8, ws * 8), np.float32))
    assert len(eng.stage_losses(touts, kmaps, pmaps, mask)) == len(touts)
    grads, _ = eng.stage_backward(kmaps, pmaps, mask)
    eng.adam_step(eng.flat_of(grads), 1e-6)


def use_and_close(dtype, shapes, base):
    fp32 = dtype == _lib.F32
    eng = Engine(0, dtype=dtype)
    try:
        eng.load_state_dict(synth.make_state_dict())
        eng.set_tracking(Engine.TRACK_LANES)
        eng.set_overlay(2)
        before_last = None
        for shape in shapes:
            before_last = live()
            one_pass(eng, shape, fp32)
        after_last = live()
        assert all(a > b for a, b in zip(after_last, base)), (after_last, base)        # (a)
        if len(shapes) == 3:                                                          # (b) A again after B: nothing re-allocated
            assert after_last[:2] == before_last[:2], (before_last, after_last)
        eng.set_capacity(1024, 64, 2048, 128)
        N, H, W = shapes[-1]
        quiet(eng.infer_poses, np.zeros((N, 3, H, W), np.float32))
        # seventeen more destination sizes: the 16-entry table cache drops its oldest geometries
        maps = np.zeros((1, 19, 4, 6), np.float32)
        for i in range(17):
            eng.multiscale_accumulate(np.zeros((1, 16 + i, 24, 19), np.float32), maps, 4, [0, 0, 0, 0], 1, init=True)
        assert all(a > b for a, b in zip(live(), base))
    finally:
        eng.h.close()
    assert live() == base                                                             # (c), (d)


@pytest.mark.parametrize("dtype", [_lib.F32, _lib.BF16], ids=["fp32", "bf16"])
def test_a_closed_engine_has_given_back_everything(dtype):
    gc.collect()                                       # engines earlier tests dropped without closing go now, not in the middle
    base = live()                                      # read before anything is created
    use_and_close(dtype, [SHAPE_A, SHAPE_B, SHAPE_A], base)
    use_and_close(dtype, [SHAPE_A], base)              # a second create / use / close cycle ends at the same reading
