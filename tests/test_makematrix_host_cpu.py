"""The host half of -makematrix (veryfasttree_amd/host/SeqMatrix.h: row pool, slab ranges, double buffering, "%f" text) on the CPU
against a fake slab source - a stand-alone program (tests/native/seqmatrix_host_check.cpp), once plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU or code loaded into Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True])
def test_slab_driver_against_a_fake_source(tmp_path, sanitize):
    exe = str(tmp_path / "smcheck")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++11", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "seqmatrix_host_check.cpp"), "-o", exe, "-pthread"],
                   check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("failures 0") and "refused (Non-unique name" in out, out[-3000:]
