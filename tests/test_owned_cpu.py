"""The allocation owner of a context (veryfasttree_amd/csrc/vft_owned.h) as a stand-alone program over malloc / free
(tests/native/owned_check.cpp): groups failing at every position roll back to their mark, release by pointer, regrow, release-everything
and the refusal of unknown pointers - once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; nothing
here touches a GPU or code loaded into Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_owner_as_a_stand_alone_program(tmp_path, sanitize):
    exe = str(tmp_path / "ownedcheck")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "owned_check.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("failures 0"), out[-3000:]
