"""The argument layouts and the stale-node collector of the C ABI (veryfasttree_amd/csrc/vft_staging.h) as a stand-alone program
(tests/native/staging_check.cpp): regions that never overlap and honour their alignment, the list length at which every dual-path entry
point leaves the host-mapped ring for the device scratch, and the collector's distinct stale ids in first-seen order across an epoch wrap -
once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU or code loaded into
Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_staging_as_a_stand_alone_program(tmp_path, sanitize):
    exe = str(tmp_path / "stagingcheck")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "staging_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("failures 0"), out[-3000:]
