"""GPU: the crowd-mask kernel (csrc/crowd_kernels.hip) through Engine.crowd_masks against the loop restatement of
crowd_mask_cases.py on its case table, and through Engine.augment_batch / val.augmented_train_step against the existing route
fed the NumPy-decoded float masks.  The values are 0.0 and 1.0 and the augmentation behind them is integer or fixed-order
float32: everything is compared bit for bit.  The restatement is unpinned against pycocotools itself."""
import ctypes
import gc
import random

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, optim, synth, val
from lwpose_amd.datasets import transformations as T
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import augment_cases as ac
import crowd_mask_cases as cm

pytestmark = pytest.mark.gpu
PAD = (128, 128, 128)


@pytest.fixture(scope="module")
def eng():
    return Engine(0, nref=1, num_channels=32)          # neither call needs weights


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)


def assert_masks(got, want):
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, n
        assert torch.equal(g.cpu(), torch.from_numpy(w)), "image %d: %d pixels differ" % (n, int((g.cpu().numpy() != w).sum()))


@pytest.mark.parametrize("name", list(cm.CASES))
def test_crowd_masks_equal_the_restatement(eng, name):
    sizes, segs, want = cm.case(name)
    got = eng.crowd_masks(segs, sizes)
    assert_masks(got, want)
    base = got[0].untyped_storage().data_ptr()         # views of ONE buffer, image after image
    at = 0
    for g, (h, w) in zip(got, sizes):
        assert g.untyped_storage().data_ptr() == base and g.storage_offset() == at and g.is_contiguous()
        at += h * w


def test_the_whole_table_as_one_batch(eng):
    """Every case in one launch: 30-odd images of different sizes, LDS and global tables side by side, the output offsets."""
    sizes, segs, want = [], [], []
    for name in cm.CASES:
        s, g, w = cm.case(name)
        sizes, segs, want = sizes + s, segs + g, want + w
    got = eng.crowd_masks(segs, sizes)
    assert_masks(got, want)
    again = eng.crowd_masks(segs, sizes)               # repeatability: the same bits
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    assert eng.crowd_masks(segs, sizes, time_iters=2) > 0


def test_a_caller_stream_sees_the_finished_masks_without_a_host_synchronise(eng):
    """The engine orders its stream against torch's current one (lwp_set_stream): a copy queued on the caller's side stream
    right behind the call reads finished masks."""
    sizes, segs, want = cm.case("45x131")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        copies = [m.clone() for m in eng.crowd_masks(segs * 8, sizes * 8)]
    side.synchronize()
    assert_masks(copies, want * 8)


def segmentation_batch():
    """12 samples: mixed sizes, host and cuda images, segmentations / None / []; and the same with decoded float masks."""
    with_segs, with_masks = [], []
    for n in range(12):
        h, w = 11 + 5 * (n % 5), 70 - 4 * n
        s = ac.synthetic_sample(800 + n, h, w, others=n % 3, scale_provided=float(0.15 + 0.02 * n), with_mask=False)
        del s["mask"]
        segs = None if n % 3 == 1 else [] if n % 3 == 2 else [cm.rle_encode(cm.blob_grid(h, w, 60 + n)), cm.rle([h + 1, 3 * h, 2, h], h, w)]
        mask = cm.get_mask_ref(segs, np.ones((h, w), dtype=np.float32)) if segs else None
        image = s["image"]
        if n % 4 >= 2:                                 # resident in device memory: read in place
            image = torch.from_numpy(image).cuda()
            mask = None if mask is None else torch.from_numpy(mask).cuda()
        with_segs.append(dict(s, image=image, segmentations=segs))
        with_masks.append(dict(s, image=image, mask=mask))
    return with_segs, with_masks


def test_augment_batch_from_segmentations_equals_the_float_mask_route_and_the_host(eng):
    with_segs, with_masks = segmentation_batch()
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=PAD), T.CropPad(pad=(1, 2, 3), center_perterb_max=10, crop_x=72, crop_y=40),
                  T.Flip()]
    plan = T.plan_batch(with_segs, transforms, random.Random(33))
    plan_masks = T.plan_batch(with_masks, transforms, random.Random(33))
    assert sum(bool(s) for s in plan.segmentations) == 4 and plan_masks.segmentations is None
    host = T.apply_plan_host(plan, 8)
    assert 0 < int((host[1] == 0).sum()) and np.any(host[2] == 0) and np.any(host[2] == 1)
    got = eng.augment_batch(plan)
    want = eng.augment_batch(plan_masks)
    again = eng.augment_batch(plan)
    for name, g, w, a, hst in zip(("image", "mask", "mask_small"), got, want, again, host):
        assert g.dtype == w.dtype and torch.equal(g, w), name
        assert torch.equal(g, a), name
        assert torch.equal(g.cpu(), torch.from_numpy(hst)), name
    with pytest.raises(ValueError, match="timing twin"):
        eng.augment_batch(plan, time_iters=2)
    assert eng.augment_batch(plan_masks, time_iters=2) > 0


def make_net(seed=21):
    sd = synth.make_state_dict(1, seed=seed, num_channels=32, num_heatmaps=19, num_pafs=38)
    net = PoseEstimationWithMobileNet(num_refinement_stages=1, num_channels=32, num_heatmaps=19, num_pafs=38)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    return net


def test_augmented_train_step_from_segmentations_equals_the_step_from_decoded_masks():
    with_segs, with_masks = [], []
    for n in range(2):
        h, w = 30 + 4 * n, 41 - 3 * n
        s = ac.synthetic_sample(300 + n, h, w, others=n, scale_provided=0.5, with_mask=False)
        del s["mask"]
        grid = np.zeros((h, w), dtype=bool)
        grid[h // 4:h // 2 + 3, w // 3:w // 3 + 12] = True
        segs = [cm.rle_encode(grid)]
        with_segs.append(dict(s, segmentations=segs))
        with_masks.append(dict(s, mask=cm.get_mask_ref(segs, np.ones((h, w), dtype=np.float32))))
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=PAD), T.CropPad(pad=PAD, center_perterb_max=5, crop_x=32, crop_y=32), T.Flip()]
    net_a, net_b = make_net(), make_net()
    opt_a, opt_b = optim.StageAdam(net_a, base_lr=1e-3), optim.StageAdam(net_b, base_lr=1e-3)
    small = T.apply_plan_host(T.plan_batch(with_segs, transforms, random.Random(9)), 8)[2]
    assert np.any(small == 0) and np.any(small == 1)                     # the crowd region takes part in the loss
    losses_a = val.augmented_train_step(net_a, opt_a, with_segs, T.DeviceAugment(transforms, rng=random.Random(9)))
    losses_b = val.augmented_train_step(net_b, opt_b, with_masks, T.DeviceAugment(transforms, rng=random.Random(9)))
    assert losses_a == losses_b and all(np.isfinite(losses_a)) and sum(losses_a) > 0
    flat_a = net_a.engine.flat_of(net_a.engine.stage_params())
    assert torch.equal(flat_a, net_b.engine.flat_of(net_b.engine.stage_params()))


def test_a_closed_engine_has_given_back_what_the_crowd_calls_took():
    gc.collect()
    base = live()
    e = Engine(0, nref=1, num_channels=32)
    try:
        sizes, segs, want = cm.case("mixed_sizes")
        assert_masks(e.crowd_masks(segs, sizes), want)
        assert live()[0] > base[0]
        with_segs, _ = segmentation_batch()
        transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=PAD), T.CropPad(pad=PAD, center_perterb_max=10, crop_x=72, crop_y=40),
                      T.Flip()]
        e.augment_batch(with_segs, transforms, random.Random(33))
        grown = live()
        e.augment_batch(with_segs, transforms, random.Random(33))
        assert_masks(e.crowd_masks(segs, sizes), want)
        assert live() == grown                                           # grow-only: the second round allocates nothing
    finally:
        e.h.close()
    assert live() == base
