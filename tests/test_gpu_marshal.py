"""GPU: the marshalling contract of ``runtime.Engine`` at tiny sizes.  The same data handed over as a numpy array, as a cuda
tensor and as a non-contiguous view gives the same bytes; a cuda tensor of the wrong element type or on another GPU, and a
read before any result exists, raise instead of reading memory as something it is not."""
import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import synth
from lwpose_amd.runtime import Engine

pytestmark = pytest.mark.gpu

K = 18


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.load_state_dict(synth.make_state_dict(1))
    return e


@pytest.fixture(scope="module")
def data():
    """A 2 x 3 x 32 x 48 input, 8 x 12 maps with a few peaks, a 2 x 24 x 40 mask and 24 x 40 x 3 uint8 frames; ``wide``
    holds each in a buffer with spare columns, so that ``wide[k][..., :w]`` is a non-contiguous view of the same values."""
    d = {"x": synth.uniform((2, 3, 32, 48), 11, -0.5, 0.5),
         "maps": synth.uniform((2, 19, 8, 12), 12, 0.0, 0.05),
         "paf": synth.uniform((2, 38, 8, 12), 13, -0.05, 0.05),
         "mask": synth.uniform((2, 24, 40), 14),
         "frames": synth.make_frames(2, 24, 40)}
    for f, k, y, x in ((0, 0, 2, 3), (0, 1, 5, 8), (1, 4, 3, 6), (1, 17, 6, 2)):
        d["maps"][f, k, y, x] = 0.9
    d["wide"] = {}
    for key, axis in (("x", 3), ("maps", 3), ("paf", 3), ("mask", 2), ("frames", 2)):
        a = d[key]
        pad = np.zeros(a.shape[:axis] + (5,) + a.shape[axis + 1:], a.dtype)
        d["wide"][key] = np.concatenate([a, pad], axis=axis)
    kp = np.full((2, K, 2), -1, np.int32)
    kp[0, :6] = [[5, 4], [20, 6], [30, 18], [8, 20], [12, 11], [35, 3]]
    kp[1, 3:9] = [[3, 3], [10, 15], [25, 20], [38, 22], [17, 9], [1, 12]]
    d["kp"], d["bbox"] = kp, np.array([[4, 2, 30, 18], [1, 3, 37, 19]], np.int32)
    return d


def view(d, key):
    """The non-contiguous view of ``d[key]``."""
    axis = {"mask": 2, "frames": 2}.get(key, 3)
    v = d["wide"][key][(slice(None),) * axis + (slice(0, d[key].shape[axis]),)]
    assert not v.flags.c_contiguous and np.array_equal(v, d[key])
    return v


def cuda_view(d, key):
    axis = {"mask": 2, "frames": 2}.get(key, 3)
    v = torch.from_numpy(d["wide"][key]).cuda()[(slice(None),) * axis + (slice(0, d[key].shape[axis]),)]
    assert not v.is_contiguous()
    return v


def host(r):
    """A result as nested tuples of bytes and scalars: equal means identical bytes, shapes and types."""
    if isinstance(r, torch.Tensor):
        r = r.cpu().numpy()
    if isinstance(r, np.ndarray):
        return (r.dtype.str, r.shape, r.tobytes())
    if isinstance(r, (list, tuple)):
        return tuple(host(v) for v in r)
    return r


def run_forward(e, d, x):
    return e.forward(x)


def run_upsample(e, d, x):
    return e.upsample(x, 4)


def run_poses(e, d, x):
    paf = d["paf"] if isinstance(x, np.ndarray) else torch.from_numpy(d["paf"]).cuda()
    out = e.poses_from_maps(x, paf, upsample_ratio=4)
    assert sum(len(f[1]) for f in out) >= 4              # the planted peaks are found: the comparison is of real rows
    return out


def run_accumulate(e, d, x):
    return e.multiscale_accumulate(np.zeros((2, 24, 40, 19), np.float32), x, 4, [0, 0, 2, 4], 2, init=True)


def run_mask(e, d, x):
    return e.mask_downsample(x, 8)


def run_pre(e, d, x):
    return e.preprocess_u8(x[0], 32, 8)


def run_pre_batch(e, d, x):
    return e.preprocess_u8_batch(x, 32, 8)


def run_draw(e, d, x):
    return e.draw_poses(x, d["kp"][:, None], d["bbox"][:, None], n_poses=[1, 1], device_out=False)


CALLS = {"forward": (run_forward, "x"), "upsample": (run_upsample, "maps"), "poses_from_maps": (run_poses, "maps"),
         "multiscale_accumulate": (run_accumulate, "maps"), "mask_downsample": (run_mask, "mask"), "preprocess_u8": (run_pre, "frames"),
         "preprocess_u8_batch": (run_pre_batch, "frames"), "draw_poses": (run_draw, "frames")}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_numpy_cuda_and_strided_inputs_give_the_same_bytes(eng, data, name):
    run, key = CALLS[name]
    want = host(run(eng, data, data[key]))
    assert host(run(eng, data, torch.from_numpy(data[key]).cuda())) == want
    assert host(run(eng, data, view(data, key))) == want
    assert host(run(eng, data, cuda_view(data, key))) == want


def test_accum_on_the_device_is_updated_in_place(eng, data):
    want = run_accumulate(eng, data, data["maps"])
    acc = torch.empty((2, 24, 40, 19), dtype=torch.float32, device="cuda")
    assert eng.multiscale_accumulate(acc, torch.from_numpy(data["maps"]).cuda(), 4, [0, 0, 2, 4], 2, init=True) is acc
    assert host(acc) == host(want)
    with pytest.raises(TypeError, match="accum must be a contiguous float32 tensor"):
        eng.multiscale_accumulate(acc.double(), data["maps"], 4, [0, 0, 2, 4], 2, init=True)


def test_float64_cuda_maps_are_refused(eng, data):
    maps64, paf = torch.from_numpy(data["maps"]).cuda().double(), torch.from_numpy(data["paf"]).cuda()
    with pytest.raises(TypeError):
        eng.upsample(maps64, 4)
    with pytest.raises(TypeError):
        eng.multiscale_accumulate(np.zeros((2, 24, 40, 19), np.float32), maps64, 4, [0, 0, 2, 4], 2, init=True)
    for heat, p in ((maps64, paf), (maps64.float(), paf.half())):
        with pytest.raises(TypeError):
            eng.poses_from_maps(heat, p)
        with pytest.raises(TypeError):
            eng.coco_add_maps(heat, p, [0, 1])
    # host arrays of another type are converted, as they always were
    assert host(eng.upsample(data["maps"].astype(np.float64), 4)) == host(eng.upsample(data["maps"], 4))


def test_reads_before_any_result_name_the_missing_call():
    e = Engine(0)
    for call in (e.fetch_poses, e.poses, lambda: e.pipeline_fetch(0), lambda: e.poses(1), lambda: e.pipeline_overlay(0)):
        with pytest.raises(RuntimeError, match="call "):
            call()
    assert e.caps == (2048, 128, 4096, 256)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_tensor_on_another_gpu_is_refused(eng, data, name):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU")
    run, key = CALLS[name]
    with pytest.raises(ValueError, match="on cuda:1 but the engine lives on cuda:0"):
        run(eng, data, torch.from_numpy(data[key]).to("cuda:1"))
