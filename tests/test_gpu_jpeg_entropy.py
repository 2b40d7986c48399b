"""GPU: the device entropy decoder of the JPEG reader (csrc/jpeg_entropy_kernels.hip behind lwp_set_jpeg_entropy) against the
host decoder of the same library, bit for bit: coefficients of every fixture and of synthetic streams from the encoder of
jpeg_entropy_cases at several subsequence sizes, pixels against Pillow's, every single-bit flip of two scans (the CPU test
test_jpeg_entropy_host.py runs the restated algorithm with bounds assertions over the same set), the call contract of
decode_jpeg_batch in device mode, and the training data path."""
import ctypes
import gc
import os
import random

import numpy as np
import pytest
import torch

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib, demo
from lwpose_amd.datasets import coco
from lwpose_amd.datasets import transformations as T
from lwpose_amd.runtime import Engine

import augment_cases as ac
import crowd_mask_cases as cm
import jpeg_cases as jc
import jpeg_entropy_cases as je

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
FIX = jc.fixtures()
NAMES = sorted(FIX)
PAD = (128, 128, 128)
SIZES = (4, 8, 32, 0)                                  # 0: the default


@pytest.fixture(scope="module")
def eng():
    return Engine(0, nref=1, num_channels=32)          # the decode needs no weights


@pytest.fixture(scope="module")
def real():
    with np.load(os.path.join(GOLDEN, "jpeg_extra.npz")) as z:
        return z["jpeg"].tobytes()


@pytest.fixture(scope="module")
def host(real):
    """{bytes: (coefficients, tables)} by the host decoder, computed once."""
    out = {}
    for data in [FIX[n][0] for n in NAMES] + [real] + list(je.synthetic().values()):
        _, coef, qt = Engine.debug_jpeg_blocks(data)
        out[data] = (coef, qt)
    return out


def live():
    out = (ctypes.c_int64 * 4)()
    assert _lib.lib().lwp_debug_live_resources(out) == _lib.LWP_OK
    return tuple(int(v) for v in out)


def check_equal(got, files, host, what):
    assert len(got) == len(files)
    for k, ((status, coef, qt), data) in enumerate(zip(got, files)):
        want_coef, want_qt = host[data]
        assert status == 0, "%s: file %d refused" % (what, k)
        assert coef.shape == want_coef.shape and np.array_equal(coef, want_coef), "%s: file %d: %d coefficients differ" % (
            what, k, int((coef != want_coef).sum()))
        assert np.array_equal(qt, want_qt), "%s: file %d: tables differ" % (what, k)


@pytest.mark.parametrize("subseq", SIZES)
def test_fixture_coefficients_equal_the_host_decoder(eng, real, host, subseq):
    files = [FIX[n][0] for n in NAMES] + [real]
    batch = eng.debug_jpeg_entropy(files, subseq)
    check_equal(batch, files, host, "one batch")
    check_equal(eng.debug_jpeg_entropy(files, subseq), files, host, "again")
    check_equal(eng.debug_jpeg_entropy(files[::-1], subseq), files[::-1], host, "reversed")
    for f in files:
        check_equal(eng.debug_jpeg_entropy([f], subseq), [f], host, "alone")


@pytest.mark.parametrize("subseq", (4, 0))
def test_synthetic_streams_equal_the_host_decoder(eng, host, subseq):
    syn = je.synthetic()
    assert len(je.scan_bytes(syn["big_420"])) > 3 * 256 * je.DEFAULT_SUBSEQ
    files = list(syn.values())
    check_equal(eng.debug_jpeg_entropy(files, subseq), files, host, "synthetic")
    for name, f in syn.items():
        check_equal(eng.debug_jpeg_entropy([f], subseq), [f], host, name)


def differing(t, want):
    return int((t.cpu().numpy() != want).sum())


def test_pixels_in_device_mode_equal_pillow_and_the_host_mode(eng):
    got = eng.decode_jpeg_batch([FIX[n][0] for n in NAMES], entropy="device")
    for name, img in zip(NAMES, got):
        assert differing(img, FIX[name][1]) == 0, name
    files = list(je.synthetic().values())
    want = eng.decode_jpeg_batch(files)
    got = eng.decode_jpeg_batch(files, entropy="device")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    a_ms, b_ms = eng.decode_jpeg_batch(files, time_iters=2, entropy="device")
    assert a_ms > 0 and b_ms > 0
    again = eng.decode_jpeg_batch(files, entropy="device")
    assert all(torch.equal(a, b) for a, b in zip(again, want))


@pytest.mark.parametrize("name", ["17x17_420", "restart2_33x16_422"])
def test_bit_flip_mutants_get_the_host_verdict(eng, host, name):
    """One batch per source file.  test_jpeg_entropy_host.py runs the restated kernels, which assert the bounds of every read
    and store, over the same mutants."""
    mutants = list(je.bit_flips(FIX[name][0]))
    want = []
    for m in mutants:
        try:
            want.append(Engine.debug_jpeg_blocks(m)[1:])
        except ValueError:
            want.append(None)
    assert any(w is None for w in want) and any(w is not None for w in want)
    for subseq in (4, 0):
        got = eng.debug_jpeg_entropy(mutants, subseq)
        for k, ((status, coef, qt), w) in enumerate(zip(got, want)):
            assert (status == 0) == (w is not None), "mutant %d at %d: device %d, host %s" % (k, subseq, status, "accepts" if w else "refuses")
            if w is not None:
                assert np.array_equal(coef, w[0]) and np.array_equal(qt, w[1]), "mutant %d at %d" % (k, subseq)
    clean = [FIX[n][0] for n in NAMES[:8]]
    check_equal(eng.debug_jpeg_entropy(clean), clean, host, "a clean batch afterwards")


def decode_into(eng, files, outs):
    n = len(files)
    data = (ctypes.c_void_p * n)(*[ctypes.cast(ctypes.c_char_p(f), ctypes.c_void_p) for f in files])
    lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    rc = _lib.lib().lwp_jpeg_decode_batch(eng.h.ptr, n, data, lens, ptrs)
    return rc, _lib.lib().lwp_last_error(eng.h.ptr).decode()


def test_a_refused_file_in_device_mode_fails_the_call_as_in_host_mode_and_writes_nothing():
    e = Engine(0, nref=1, num_channels=32)
    names = ["17x17_420", "33x16_422", "grey_19x21", "9x31_444"]
    files = [FIX[n][0] for n in names]
    outs = [torch.full(FIX[n][1].shape, 7, dtype=torch.uint8, device="cuda") for n in names]
    torch.cuda.synchronize()
    truncated = files[2][:-9] + b"\xff\xd9"            # refused by the kernels: the data ends before the last MCU
    no_eoi = files[3][:-2]                             # refused by the pre-pass
    flipped = next(m for m in je.bit_flips(files[0]) if not _accepted(m))
    for bad in ([files[0], files[1], truncated, no_eoi], [files[0], flipped, files[2], truncated], [no_eoi] + files[1:]):
        rc_host, msg_host = decode_into(e, bad, outs)
        e.set_jpeg_entropy("device", 8)
        rc, msg = decode_into(e, bad, outs)
        e.set_jpeg_entropy("host")
        assert rc == rc_host == _lib.LWP_ERR_ARG and msg == msg_host and msg.startswith("image "), (msg, msg_host)
        with pytest.raises(ValueError) as err:
            e.decode_jpeg_batch(bad, entropy="device")
        assert str(err.value) == msg_host
    e.synchronize()
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in outs)
    e.set_jpeg_entropy("device")
    rc, msg = decode_into(e, files, outs)               # and the handle is fine afterwards
    assert rc == _lib.LWP_OK, msg
    torch.cuda.synchronize()
    assert all(differing(o, FIX[n][1]) == 0 for n, o in zip(names, outs))
    e.h.close()


def _accepted(data):
    try:
        Engine.debug_jpeg_blocks(data)
        return True
    except ValueError:
        return False


def test_a_caller_stream_sees_the_finished_pixels_in_device_mode(eng):
    files = [FIX[n][0] for n in NAMES] * 2
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        copies = [img.clone() for img in eng.decode_jpeg_batch(files, entropy="device")]
    side.synchronize()
    assert all(differing(c, FIX[n][1]) == 0 for c, n in zip(copies, NAMES * 2))


def test_a_closed_engine_has_given_back_what_the_device_mode_took():
    gc.collect()
    base = live()
    e = Engine(0, nref=1, num_channels=32)
    try:
        created = live()
        e.set_jpeg_entropy("device", 32)
        imgs = e.decode_jpeg_batch([FIX[n][0] for n in NAMES[:6]])
        grown = live()
        assert grown[0] > created[0] and grown[1] > created[1]          # the workspace and the pinned staging are counted
        again = e.decode_jpeg_batch([FIX[n][0] for n in NAMES[:6]])
        assert live() == grown                          # a second batch of the same size takes nothing more
        assert all(torch.equal(a, b) for a, b in zip(again, imgs)) and differing(imgs[0], FIX[NAMES[0]][1]) == 0
    finally:
        e.h.close()
    assert live() == base


def test_set_jpeg_entropy_rejects_bad_arguments(eng):
    L = _lib.lib()
    for mode, subseq in ((2, 0), (-1, 0), (1, 2), (1, 6), (1, 1028), (1, -4), (0, 130)):
        assert L.lwp_set_jpeg_entropy(eng.h.ptr, mode, subseq) == _lib.LWP_ERR_ARG, (mode, subseq)
    assert L.lwp_set_jpeg_entropy(None, 1, 0) == _lib.LWP_ERR_ARG
    for mode, subseq in ((1, 4), (1, 1024), (1, 0), (0, 0)):
        assert L.lwp_set_jpeg_entropy(eng.h.ptr, mode, subseq) == _lib.LWP_OK
    with pytest.raises(ValueError):
        eng.set_jpeg_entropy("gpu")
    with pytest.raises(ValueError):
        eng.set_jpeg_entropy("device", 5)
    with pytest.raises(ValueError):
        eng.decode_jpeg_batch([FIX[NAMES[0]][0]], entropy="gpu")
    with pytest.raises(ValueError):
        eng.debug_jpeg_entropy([FIX[NAMES[0]][0]], 7)


def test_train_dataset_in_device_mode_gives_the_bits_of_the_host_mode(eng, tmp_path):
    names = ["large_100x75_420", "37x53_422"]
    labels = []
    for n, name in enumerate(names):
        with open(os.path.join(str(tmp_path), name + ".jpg"), "wb") as f:
            f.write(FIX[name][0])
        h, w = FIX[name][1].shape[:2]
        label = ac.synthetic_sample(500 + n, h, w, others=n, scale_provided=0.5, with_mask=False)["label"]
        grid = np.zeros((h, w), dtype=bool)
        grid[h // 4:h // 2 + 3, w // 3:w // 3 + 12] = True
        label.update(img_paths=name + ".jpg", segmentations=[cm.rle_encode(grid)])
        labels.append(label)
    transforms = [T.ConvertKeypoints(), T.Scale(), T.Rotate(pad=PAD), T.CropPad(pad=PAD, center_perterb_max=5, crop_x=48, crop_y=40), T.Flip()]
    out = {}
    for mode in ("host", "device"):
        samples = coco.CocoTrainDataset(labels, str(tmp_path), eng, entropy=mode).samples([0, 1])
        assert all(differing(s["image"], FIX[n][1]) == 0 for s, n in zip(samples, names))
        out[mode] = T.DeviceAugment(transforms, engine=eng, rng=random.Random(5))(samples)
    for key in ("image", "mask", "mask_small"):
        assert torch.equal(out["host"][key], out["device"][key]), key
    path = os.path.join(str(tmp_path), names[0] + ".jpg")
    assert differing(coco.imread(path, eng, entropy="device"), FIX[names[0]][1]) == 0
    frames = list(demo.ImageReader([path], eng, entropy="device"))
    assert len(frames) == 1 and differing(frames[0], FIX[names[0]][1]) == 0
