"""The `-intree` parser (veryfasttree_amd/host/ReadTree.h) as a stand-alone program (tests/native/read_tree_check.cpp): its built-in well-formed
and malformed texts, a million nested parentheses, a long caterpillar, and three fixture texts whose node arrays must hash to the fixture's -
once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; nothing here touches a GPU or code loaded into
Python)."""
import os
import re
import subprocess

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["intree_nt_5", "intree_nt_200_me", "intree_nt_62_dups_caterpillar"]


def fnv1a(arrays):
    h = 1469598103934665603
    for a in arrays:
        for b in np.ascontiguousarray(a, "<i8").tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def write_case(path, d):
    codes = d["codes"]
    first_of, to_uniq, first = {}, [], []
    for k, row in enumerate(codes):
        if row.tobytes() not in first_of:
            first_of[row.tobytes()] = len(first)
            first.append(k)
        to_uniq.append(first_of[row.tobytes()])
    with open(path, "wb") as fh:
        fh.write(("%d %d\n" % (len(codes), len(first))).encode())
        fh.write("".join("s%d %d\n" % (k, u) for k, u in enumerate(to_uniq)).encode())
        fh.write((" ".join(str(k) for k in first) + "\n").encode())
        fh.write(bytes(d["intree"]))


@pytest.mark.parametrize("sanitize", [False, True])
def test_parser_as_a_stand_alone_program(tmp_path, sanitize):
    exe = str(tmp_path / "rtcheck")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++11", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "read_tree_check.cpp"), "-o", exe], check=True)
    files = []
    for name in CASES:
        files.append(str(tmp_path / name))
        write_case(files[-1], G.load(name))
    res = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("failures 0"), out[-3000:]
    assert "refused (The starting tree must be binary" in out and "refused (Tree parse error" in out
    for name in CASES:
        d = G.load(name)
        m = re.search(r"^case %s root (\d+) nodes (\d+) digest ([0-9a-f]{16})$" % name, out, re.M)
        assert m, out[-3000:]
        assert (int(m.group(1)), int(m.group(2))) == (int(d["root"]), len(d["parent"]))
        assert int(m.group(3), 16) == fnv1a([d["parent"], d["child"]])
