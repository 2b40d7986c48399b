"""CPU: the device entropy decoder of the JPEG reader without a GPU.  The encoder of jpeg_entropy_cases against the fixtures'
own scan bytes and against the restated decoder; the host pre-pass (lwp_debug_jpeg_scan) against its restatement on every
fixture and every single-bit flip of two scans, and in a stand-alone program under the host compiler's sanitizers; the
restated kernels (which assert the bounds of every read and store) against the host decoder on the fixtures, the synthetic
streams and the same bit flips; and mutated restatements that the streams must tell from the right one."""
import os
import re
import subprocess

import numpy as np
import pytest

import lwpose_amd  # noqa: F401
from lwpose_amd import _lib
from lwpose_amd.runtime import Engine

import jpeg_cases as jc
import jpeg_entropy_cases as je
from test_jpeg_host import host_compiler_with_sanitizers

from conftest import GOLDEN, ROOT

NEW_EXPORTS = ["lwp_set_jpeg_entropy", "lwp_debug_jpeg_entropy_batch", "lwp_debug_jpeg_scan", "lwp_time_jpeg_entropy_batch"]
FIX = jc.fixtures()
FLIPPED = ("17x17_420", "restart2_33x16_422")
SAMPLING = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}


def host_verdict(data):
    """(coefficients, tables) of the library's host decoder, None where it refuses."""
    try:
        return Engine.debug_jpeg_blocks(data)[1:]
    except ValueError:
        return None


@pytest.fixture(scope="module")
def flips():
    """{name: [(mutant, host verdict)]} of every single-bit flip of the scans of FLIPPED, computed once."""
    return {name: [(m, host_verdict(m)) for m in je.bit_flips(FIX[name][0])] for name in FLIPPED}


def test_new_exports_are_declared_and_present():
    L = _lib.lib()
    with open(os.path.join(ROOT, "include", "lwpose.h")) as f:
        declared = set(re.findall(r"\b(lwp_[a-z_0-9]+)\s*\(", f.read()))
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name in declared, name
    assert L.lwp_set_jpeg_entropy(None, 0, 0) == _lib.LWP_ERR_ARG


# ------------------------------------------------------------------------------------------------ the encoder
def test_encoder_reproduces_the_scan_bytes_of_the_fixtures_with_standard_tables():
    std = je.standard_tables()
    n = 0
    for name, (data, _) in FIX.items():
        tables, _ = je.raw_tables(data)
        if any(tables.get(k) != std[k] for k in tables) or b"\xff\xff" in je.scan_bytes(data):
            continue                                   # optimised tables; fill bytes in front of a marker
        hd, coef, qt = jc.restated(name)
        sampling = "grey" if hd["components"] == 1 else SAMPLING[(hd["h_samp"][0], hd["v_samp"][0])]
        g = je.geometry(hd["width"], hd["height"], sampling)
        assert all(g[k] == hd[k] for k in g), name
        assert je.encode_scan(coef, g, tables, hd["td"], hd["ta"], hd["restart_interval"]) == je.scan_bytes(data), name
        n += 1
    assert n > 25


@pytest.mark.parametrize("name", sorted(je.synthetic()))
def test_encoded_streams_decode_to_their_coefficients(name):
    data = je.synthetic()[name]
    hd, coef, qt = Engine.debug_jpeg_blocks(data)
    if len(data) < 30000:                              # the NumPy restatement is slow; the library's host decoder is pinned to it
        assert np.array_equal(jc.decode_blocks(data)[1], coef)
    sampling = "grey" if hd["components"] == 1 else SAMPLING[(hd["h_samp"][0], hd["v_samp"][0])]
    tables, _ = je.raw_tables(data)
    again = je.encode(coef, hd["width"], hd["height"], sampling, tables, restart_interval=hd["restart_interval"])
    assert again == data


def test_encoder_round_trip_of_random_coefficients():
    std = je.standard_tables()
    for seed, (w, h, sampling, ri) in enumerate([(17, 9, "420", 0), (33, 16, "422", 2), (8, 24, "444", 1), (21, 19, "grey", 3)]):
        g = je.geometry(w, h, sampling)
        coef = je.random_coefficients(40 + seed, g, density=0.4)
        data = je.encode(coef, w, h, sampling, std, restart_interval=ri)
        assert np.array_equal(jc.decode_blocks(data)[1], coef)
        assert np.array_equal(Engine.debug_jpeg_blocks(data)[1], coef)


# ------------------------------------------------------------------------------------------------ the pre-pass
def check_scan(data, what):
    got = Engine.debug_jpeg_scan(data)
    status, raw, segs = je.scan_segments(data)
    assert got["status"] == status, what
    if status == 0:
        assert got["bytes"] == raw and got["segments"].tolist() == [list(s) for s in segs], what
    return got


@pytest.mark.parametrize("name", sorted(FIX))
def test_pre_pass_equals_its_restatement_on_every_fixture(name):
    data = FIX[name][0]
    got = check_scan(data, name)
    assert got["status"] == 0
    hd, _, qt = jc.restated(name)
    assert np.array_equal(got["qtables"], qt)
    n_mcus = hd["mcus_x"] * hd["mcus_y"]
    assert int(got["segments"][:, 3].sum()) == n_mcus and int(got["segments"][:, 1].sum()) == len(got["bytes"])
    tables, _ = je.raw_tables(data)
    for c in range(hd["components"]):
        assert got["tables"][c].tobytes() == je.flat_table(*tables[(0, hd["td"][c])]), (name, c)
        assert got["tables"][3 + c].tobytes() == je.flat_table(*tables[(1, hd["ta"][c])]), (name, c)
    for c in range(hd["components"], 3):
        assert not got["tables"][c].any() and not got["tables"][3 + c].any()


def test_pre_pass_on_the_fixtures_with_fill_bytes_and_restarts():
    fill = Engine.debug_jpeg_scan(FIX["fill_bytes_33x16_422"][0])
    plain = Engine.debug_jpeg_scan(FIX["restart2_33x16_422"][0])
    assert fill["status"] == plain["status"] == 0 and len(plain["segments"]) > 1
    assert fill["segments"].tolist() == plain["segments"].tolist() and fill["bytes"] == plain["bytes"]
    many = Engine.debug_jpeg_scan(FIX["restart2_37x53_420"][0])
    assert many["segments"][:, 2].tolist() == list(range(0, 12, 2)) and many["segments"][:, 3].tolist() == [2] * 6


@pytest.mark.parametrize("name", FLIPPED)
def test_pre_pass_equals_its_restatement_on_every_bit_flip(flips, name):
    refused = 0
    for k, (m, host) in enumerate(flips[name]):
        got = check_scan(m, (name, k))
        refused += got["status"] != 0
        assert not (got["status"] and host is not None), (name, k)      # the pre-pass refuses nothing the host decoder accepts
    assert refused > 0


def test_pre_pass_refuses_without_a_message_and_reports_a_refused_header():
    data = FIX["17x17_420"][0]
    assert Engine.debug_jpeg_scan(data[:-2])["status"] == 1               # no EOI
    assert Engine.debug_jpeg_scan(data[:-2] + b"\xff\xd0\xff\xd9")["status"] == 1   # an RST where the file has no restart interval
    with pytest.raises(ValueError, match="progressive"):
        Engine.debug_jpeg_scan(data.replace(b"\xff\xc0", b"\xff\xc2", 1))


def test_stand_alone_pre_pass_walk_under_the_sanitizers(tmp_path):
    cxx = host_compiler_with_sanitizers(tmp_path)
    if cxx is None:
        pytest.skip("no host compiler accepts -fsanitize=address,undefined")
    pkg = os.path.join(ROOT, "lightweight-human-pose-estimation.pytorch_amd", "csrc")
    exe = str(tmp_path / "jpeg_scan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(pkg, "jpeg_host.cpp"), os.path.join(ROOT, "tools", "jpeg_scan_check.cpp"), "-o", exe], check=True)
    files = []
    for name in ("17x17_420", "fill_bytes_33x16_422", "grey_19x21", "optimised_37x53_420", "restart2_33x16_422", "1x1_444"):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(FIX[name][0])
        files.append(str(path))
    r = subprocess.run([exe] + files[:4] + ["--mutate"] + files[4:], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refused" in r.stdout and " 0 disagreements" in r.stdout


# ------------------------------------------------------------------------------------------------ the algorithm
@pytest.mark.parametrize("name", sorted(FIX))
def test_restated_kernels_equal_the_restated_decoder_on_every_fixture(name):
    _, want, _ = jc.restated(name)
    for subseq in (4, 8, 32, 128):
        status, coef = je.device_decode(FIX[name][0], subseq)
        assert status == 0 and np.array_equal(coef, want), subseq


def test_restated_kernels_on_a_real_file():
    with np.load(os.path.join(GOLDEN, "jpeg_extra.npz")) as z:
        data = z["jpeg"].tobytes()
    want = Engine.debug_jpeg_blocks(data)[1]           # pinned to the restated decoder by test_jpeg_host.py
    d = je.Decoder(data, 32)
    status, coef = d.run()
    assert status == 0 and np.array_equal(coef, want)
    assert d.rounds[1] >= 1                            # several workgroups: the sync across them ran


@pytest.mark.parametrize("name", sorted(n for n in je.synthetic() if n != "big_420"))
def test_restated_kernels_on_the_synthetic_streams(name):
    data = je.synthetic()[name]
    want = Engine.debug_jpeg_blocks(data)[1]
    for subseq in (4, 128):
        status, coef = je.device_decode(data, subseq)
        assert status == 0 and np.array_equal(coef, want), subseq


@pytest.mark.parametrize("name", FLIPPED)
def test_restated_kernels_give_the_host_verdict_on_every_bit_flip(flips, name):
    accepted = 0
    for k, (m, host) in enumerate(flips[name]):
        for subseq in (4, 128):
            status, coef = je.device_decode(m, subseq)   # raises if a read or a store leaves its buffer
            assert (status == 0) == (host is not None), (name, k, subseq)
            if host is not None:
                assert np.array_equal(coef, host[0]), (name, k, subseq)
        accepted += host is not None
    assert 0 < accepted < len(flips[name])


def test_a_stream_that_never_synchronises_is_decoded_by_the_round_caps():
    data = je.synthetic()["eob_only_grey"]             # three bits a block: a lane that starts off a block's first bit stays off
    d = je.Decoder(data, 4)
    status, coef = d.run()
    assert status == 0 and not coef.any() and d.rounds[0] == je.GROUP


# ------------------------------------------------------------------------------------------------ mutated restatements
def differs_somewhere(names, **knob):
    syn = je.synthetic()
    for name in names:
        want = Engine.debug_jpeg_blocks(syn[name])[1]
        status, coef = je.device_decode(syn[name], 4, **knob)
        if status or not np.array_equal(coef, want):
            return True
    return False


def test_a_state_comparison_that_ignores_k_is_seen():
    assert differs_somewhere(["size10_grey", "long_codes_grey"], ignore_k=True)


def test_a_state_comparison_that_ignores_the_block_index_is_seen():
    assert differs_somewhere(["block_sync_444"], ignore_block=True)


def test_a_decoder_without_the_rounds_across_workgroups_is_seen():
    assert differs_somewhere(["size10_grey", "all_ones_444"], no_stitch=True)


def test_a_dc_scan_in_plane_order_is_seen():
    assert differs_somewhere(["size10_420"], dc_plane_order=True)
