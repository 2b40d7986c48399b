"""GPU: the staging every JPEG batch goes through (jpeg_stage_begin / jpeg_stage_send in csrc/capi.cpp), in an order no other
test has: on ONE fresh engine a small batch, a large one and a small one again, so the pinned and the device buffer grow after
they were used small and are used small after they grew; calls back to back, so each waits for the copy of the one before;
both entropy modes; then encodes with a decode between them, on their own buffers of the same handle.  Every result is the
fixtures' Pillow pixels or file, byte for byte."""
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd.runtime import Engine

import jpeg_cases as jc
import jpeg_encode_cases as jen

pytestmark = pytest.mark.gpu


def test_small_large_small_batches_and_alternating_encode_and_decode_on_one_engine():
    dec, enc = jc.fixtures(), jen.fixtures()
    names = sorted(dec)
    small = min(names, key=lambda n: (dec[n][1].size, n))
    assert dec[small][1].shape == (1, 1, 3)
    eng = Engine(0, nref=1, num_channels=32)           # fresh: its JPEG buffers start empty

    def decode(batch):
        got = eng.decode_jpeg_batch([dec[n][0] for n in batch])
        assert len(got) == len(batch)
        for n, img in zip(batch, got):
            assert tuple(img.shape) == dec[n][1].shape and int((img.cpu().numpy() != dec[n][1]).sum()) == 0, n

    try:
        for mode in ("host", "device"):
            eng.set_jpeg_entropy(mode)
            for batch in ([small], names, [small], ["17x17_420"]):
                decode(batch)
        setting = (75, "4:2:0", 0)
        group = [n for n in sorted(enc) if (enc[n]["quality"], enc[n]["sampling"], enc[n]["restart"]) == setting]
        one = "noise_1x1_420_q75"
        assert one in group and len(group) >= 5 and enc[one]["bgr"].shape == (1, 1, 3)
        for batch, between in (([one], names), (group, [small]), ([one], ["17x17_420"])):
            assert eng.encode_jpeg_batch([enc[n]["bgr"] for n in batch], *setting) == [enc[n]["jpeg"] for n in batch]
            decode(between)
    finally:
        eng.h.close()
