"""CPU: the JPEG batch plans without a GPU.  Where the regions of a batch's workspace lie and what the records say is host
arithmetic that every JPEG kernel trusts without a bounds check; tools/jpeg_plan_check.cpp walks it for the decode fixtures in
both entropy forms and for the encode sizes, in a stand-alone program under the host compiler's address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

import jpeg_cases as jc
import jpeg_entropy_cases as je
from test_jpeg_host import host_compiler_with_sanitizers

from conftest import ROOT


def test_stand_alone_plan_check_under_the_sanitizers(tmp_path):
    cxx = host_compiler_with_sanitizers(tmp_path)
    if cxx is None:
        pytest.skip("no host compiler accepts -fsanitize=address,undefined")
    pkg = os.path.join(ROOT, "lightweight-human-pose-estimation.pytorch_amd", "csrc")
    exe = str(tmp_path / "jpeg_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] +
                   [os.path.join(pkg, s) for s in ("jpeg_host.cpp", "jpeg_encode_host.cpp", "jpeg_batch.cpp")] +
                   [os.path.join(ROOT, "tools", "jpeg_plan_check.cpp"), "-o", exe], check=True)
    files = []
    for name, data in sorted({**{n: d for n, (d, _) in jc.fixtures().items()}, **je.synthetic()}.items()):
        path = tmp_path / (name + ".jpg")
        path.write_bytes(data)
        files.append(str(path))
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    m = re.search(r"jpeg_plan_check: (\d+) plans of (\d+) files and 7 sizes hold, (\d+) regions named by records inside them", r.stdout)
    assert m, r.stdout
    # decode: every file alone, all, all reversed, and all around a refused file, in the host form (the last case has no
    # plan there) and the device form at two subsequence counts; encode: 7 sizes and the mixed batch, 3 samplings, 3 restart
    # intervals, host and device frames
    n = len(files)
    assert int(m.group(2)) == n and int(m.group(1)) == (n + 2) * 3 + 2 + 8 * 3 * 3 * 2 and int(m.group(3)) > 0
