"""GPU: the JPEG decode (csrc/jpeg_kernels.hip behind lwp_jpeg_decode_batch) against Pillow's pixels in the fixtures, byte for
byte: every fixture in one call, alone and again; a refused file in the middle of a batch; a caller's side stream; what a
closed engine gives back; and the two datasets feeding the augmentation and val.evaluate from files."""
import ctypes
import gc
import io
import json
import os
import random
import zlib
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo, synth, val
from lwpose_amd.datasets import coco
from lwpose_amd.datasets import transformations as T
from lwpose_amd.models.with_mobilenet import PoseEstimationWithMobileNet
from lwpose_amd.modules.load_state import load_state
from lwpose_amd.runtime import Engine

import augment_cases as ac
import coco_eval_cases as cc
import crowd_mask_cases as cm
import jpeg_cases as jc

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIX = jc.fixtures()
NAMES = sorted(FIX)
PAD = (128, 128, 128)


@pytest.fixture(scope="module")
def eng():
    return Engine(0, nref=1, num_channels=32)          # the decode needs no weights


@pytest.fixture(scope="module")
def batch(eng):
    """Every fixture in ONE call: 38 files of 1x1 .. 100x75, grey and the three samplings mixed.  Stage A takes 32 blocks a
    workgroup and stage B 1024 pixels, so nearly every image boundary falls inside a workgroup of both."""
    return eng.decode_jpeg_batch([FIX[n][0] for n in NAMES])


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)


def differing(t, want):
    return int((t.cpu().numpy() != want).sum())


def test_all_fixtures_in_one_call_equal_pillow_in_every_byte(batch):
    assert len(batch) == len(NAMES) > 30
    base = batch[0].untyped_storage().data_ptr()
    for name, img in zip(NAMES, batch):
        want = FIX[name][1]
        assert img.dtype == torch.uint8 and img.is_cuda and tuple(img.shape) == want.shape and img.is_contiguous(), name
        assert img.untyped_storage().data_ptr() == base, name          # views of ONE allocation
        assert differing(img, want) == 0, "%s: %d bytes differ" % (name, differing(img, want))


@pytest.mark.parametrize("name", NAMES)
def test_each_fixture_alone_gives_the_bits_of_the_batch(eng, batch, name):
    alone = eng.decode_jpeg_batch([FIX[name][0]])
    assert len(alone) == 1 and torch.equal(alone[0], batch[NAMES.index(name)])


def test_a_second_call_gives_the_same_bits(eng, batch):
    again = eng.decode_jpeg_batch([FIX[n][0] for n in NAMES])
    assert all(torch.equal(a, b) for a, b in zip(again, batch))
    reverse = eng.decode_jpeg_batch([FIX[n][0] for n in reversed(NAMES)])
    assert all(torch.equal(a, b) for a, b in zip(reversed(reverse), batch))
    a_ms, b_ms = eng.decode_jpeg_batch([FIX[n][0] for n in NAMES], time_iters=2)
    assert a_ms > 0 and b_ms > 0


def test_a_real_file_equals_pillow(eng):
    """688 x 618 at 4:4:4 from another encoder: 20 000 blocks, hundreds of workgroups in both stages."""
    with np.load(os.path.join(GOLDEN, "jpeg_extra.npz")) as z:
        data, window, (oy, ox), shape, crc = z["jpeg"].tobytes(), z["window"], z["origin"], tuple(z["shape"]), int(z["crc32"][0])
    img = coco.imread(data, eng)
    assert tuple(img.shape) == shape
    rgb = np.ascontiguousarray(img.cpu().numpy()[:, :, ::-1])
    assert np.array_equal(rgb[oy:oy + 256, ox:ox + 256], window)
    assert zlib.crc32(rgb.tobytes()) == crc


def test_a_batch_large_enough_for_the_host_threads(eng, batch):
    """From 256 KiB of input on the files are shared among host threads (kJpegThreadedFromBytes): four copies of the 70 KB file
    and eight small ones make twelve files for twelve threads.  The same bits, and the FIRST refused file is the one named."""
    with np.load(os.path.join(GOLDEN, "jpeg_extra.npz")) as z:
        real = z["jpeg"].tobytes()
    assert 4 * len(real) > 256 * 1024
    small = NAMES[:8]
    files = [real, FIX[small[0]][0], real] + [FIX[n][0] for n in small[1:]] + [real, real]
    got = eng.decode_jpeg_batch(files)
    alone = eng.decode_jpeg_batch([real])[0]
    for k in (0, 2, 10, 11):
        assert torch.equal(got[k], alone)
    for k, n in zip([1] + list(range(3, 10)), small):
        assert torch.equal(got[k], batch[NAMES.index(n)]), n
    bad = list(files)
    bad[9] = bad[9][:-6]
    bad[4] = bad[4].replace(b"\xff\xc4", b"\xff\xcc", 1)          # parses as DAC: refused by the header pass
    bad[7] = bad[7][:-8] + b"\xff\xd9"                            # refused by the entropy decode, like file 9
    with pytest.raises(ValueError, match="image 4: .*arithmetic"):
        eng.decode_jpeg_batch(bad)
    bad[4] = files[4]
    with pytest.raises(ValueError, match="image 7: "):
        eng.decode_jpeg_batch(bad)


def decode_into(eng, files, outs):
    n = len(files)
    data = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p) for f in files])
    lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    rc = _lib.lib().lwp_jpeg_decode_batch(eng.h.ptr, n, data, lens, ptrs)
    return rc, _lib.lib().lwp_last_error(eng.h.ptr).decode()


def test_a_refused_file_in_the_middle_fails_the_call_with_its_index_and_writes_nothing(eng):
    names = ["17x17_420", "33x16_422", "grey_19x21", "9x31_444"]
    files = [FIX[n][0] for n in names]
    outs = [torch.full(FIX[n][1].shape, 7, dtype=torch.uint8, device="cuda") for n in names]
    torch.cuda.synchronize()
    progressive = files[1].replace(b"\xff\xc0", b"\xff\xc2", 1)
    rc, msg = decode_into(eng, [files[0], progressive] + files[2:], outs)
    assert rc == _lib.LWP_ERR_ARG and msg.startswith("image 1: ") and "progressive" in msg, msg
    truncated = files[2][:-9] + b"\xff\xd9"            # its header is fine: refused by the entropy decode, behind image 0 and 1
    rc, msg = decode_into(eng, files[:2] + [truncated] + files[3:], outs)
    assert rc == _lib.LWP_ERR_ARG and msg.startswith("image 2: ") and "before the last MCU" in msg, msg
    eng.synchronize()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    with pytest.raises(ValueError, match="image 1: .*progressive"):
        eng.decode_jpeg_batch([files[0], progressive])
    rc, msg = decode_into(eng, files, outs)             # and the handle is fine afterwards
    assert rc == _lib.LWP_OK
    torch.cuda.synchronize()
    assert all(differing(o, FIX[n][1]) == 0 for n, o in zip(names, outs))


def test_a_caller_stream_sees_the_finished_pixels_without_a_host_synchronise(eng):
    files = [FIX[n][0] for n in NAMES] * 4
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        copies = [img.clone() for img in eng.decode_jpeg_batch(files)]
    side.synchronize()
    assert all(differing(c, FIX[n][1]) == 0 for c, n in zip(copies, NAMES * 4))


def test_a_closed_engine_has_given_back_what_the_decode_took():
    gc.collect()
    base = live()
    e = Engine(0, nref=1, num_channels=32)
    try:
        created = live()
        imgs = e.decode_jpeg_batch([FIX[n][0] for n in NAMES[:6]])
        grown = live()
        assert grown[0] > created[0] and grown[1] > created[1]          # the workspace and the pinned staging are counted
        e.decode_jpeg_batch([FIX[n][0] for n in NAMES[:6]])
        assert live() == grown                          # a second batch of the same size takes nothing more
        assert differing(imgs[0], FIX[NAMES[0]][1]) == 0
    finally:
        e.h.close()
    assert live() == base


def write_files(folder, names):
    paths = []
    for name in names:
        path = os.path.join(str(folder), name + ".jpg")
        with open(path, "wb") as f:
            f.write(FIX[name][0])
        paths.append(path)
    return paths


def train_labels(names):
    labels = []
    for n, name in enumerate(names):
        h, w = FIX[name][1].shape[:2]
        label = ac.synthetic_sample(500 + n, h, w, others=n, scale_provided=0.5, with_mask=False)["label"]
        grid = np.zeros((h, w), dtype=bool)
        grid[h // 4:h // 2 + 3, w // 3:w // 3 + 12] = True
        label.update(img_paths=name + ".jpg", segmentations=[cm.rle_encode(grid)])
        labels.append(label)
    return labels


def test_train_dataset_through_the_device_augment_equals_the_host_fed_pillows_pixels(eng, tmp_path):
    names = ["large_100x75_420", "37x53_422"]
    write_files(tmp_path, names)
    labels = train_labels(names)
    ds = coco.CocoTrainDataset(labels, str(tmp_path), eng)
    assert len(ds) == 2
    samples = ds.samples([0, 1])
    for s, name, label in zip(samples, names, labels):
        assert s["image"].is_cuda and s["image"].dtype == torch.uint8 and differing(s["image"], FIX[name][1]) == 0
        assert s["label"] == label and s["label"] is not label and s["segmentations"] == label["segmentations"]
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=PAD), T.CropPad(pad=PAD, center_perterb_max=5, crop_x=48, crop_y=40), T.Flip()]
    got = T.DeviceAugment(transforms, engine=eng, rng=random.Random(5))(samples)
    host_samples = [{"image": FIX[name][1], "label": label, "segmentations": label["segmentations"]} for name, label in zip(names, labels)]
    host = T.apply_plan_host(T.plan_batch(host_samples, transforms, random.Random(5)), 8)
    assert np.any(host[2] == 0) and np.any(host[2] == 1)
    for key, hst in zip(("image", "mask", "mask_small"), host):
        assert torch.equal(got[key].cpu(), torch.from_numpy(hst)), key


def test_files_outside_the_scope_name_the_file_or_go_to_the_fallback(eng, tmp_path):
    names = ["17x17_420", "33x16_422"]
    paths = write_files(tmp_path, names)
    with open(paths[1], "wb") as f:
        f.write(FIX[names[1]][0].replace(b"\xff\xc0", b"\xff\xc2", 1))
    labels = train_labels(names)
    with pytest.raises(ValueError) as e:
        coco.CocoTrainDataset(labels, str(tmp_path), eng).samples([0, 1])
    assert paths[1] in str(e.value) and "progressive" in str(e.value)
    with pytest.raises(ValueError) as e:
        coco.imread(paths[1], eng)
    assert paths[1] in str(e.value)
    calls = []

    def fallback(path):
        calls.append(path)
        return FIX[names[1]][1]
    ds = coco.CocoTrainDataset(labels, str(tmp_path), eng, fallback=fallback)
    samples = ds.samples([0, 1])
    assert calls == [paths[1]] and ds.fallbacks == 1
    assert all(differing(s["image"], FIX[n][1]) == 0 for s, n in zip(samples, names))
    frames = list(demo.ImageReader([paths[0]], eng))
    assert len(frames) == 1 and differing(frames[0], FIX[names[0]][1]) == 0


def make_net(seed=21):
    sd = synth.make_state_dict(1, seed=seed, num_channels=32, num_heatmaps=19, num_pafs=38)
    net = PoseEstimationWithMobileNet(num_refinement_stages=1, num_channels=32, num_heatmaps=19, num_pafs=38)
    load_state(net, {"state_dict": sd})
    net.eval().cuda()
    return net


def test_val_dataset_through_evaluate_equals_the_call_fed_the_fixtures_arrays(tmp_path):
    names = ["large_100x75_420", "37x53_444", "grey_19x21"]
    ids = [785, 139, 632]
    net = make_net()
    for name, i in zip(names, ids):
        with open(os.path.join(str(tmp_path), "%012d.jpg" % i), "wb") as f:
            f.write(FIX[name][0])
    kp = np.zeros((17, 3))
    kp[:, 0], kp[:, 1], kp[:, 2] = np.linspace(10, 80, 17), np.linspace(5, 60, 17), 2
    anns = [{"id": 1, "image_id": 785, "category_id": 1, "keypoints": kp.reshape(-1).tolist(), "num_keypoints": 17, "area": 3000.0,
             "iscrowd": 0, "bbox": [10.0, 5.0, 70.0, 55.0]}]
    gt = cc.dataset(ids, anns)
    for im in gt["images"]:
        im["file_name"] = "%012d.jpg" % im["id"]
    ds = coco.CocoValDataset(gt, str(tmp_path), net.engine)
    assert len(ds) == 3 and [s["file_name"] for s in ds] == [im["file_name"] for im in gt["images"]]
    assert all(s["img"].is_cuda and differing(s["img"], FIX[n][1]) == 0 for s, n in zip(ds, names))
    arrays = [{"file_name": "%012d.jpg" % i, "img": FIX[n][1]} for n, i in zip(names, ids)]
    with redirect_stdout(io.StringIO()):
        want = val.evaluate(gt, str(tmp_path / "want.json"), arrays, net, base_height=64)
        got = val.evaluate(gt, str(tmp_path / "got.json"), ds, net, base_height=64)
    assert np.array_equal(np.asarray(got), np.asarray(want), equal_nan=True)
    with open(tmp_path / "want.json") as f, open(tmp_path / "got.json") as g:
        assert json.load(f) == json.load(g)
