"""`-makematrix` without a GPU: the numpy restatement of printDistances (tests/makematrix_py.py) against the reference's own standard
output (tests/golden/mm_*.npz, produced by tools/gen_makematrix_fixtures.py from `VeryFastTree ... -makematrix`), byte for byte.
Pins the semantics - which sequences, seqDist's two branches, the two numeric_t narrowings, logCorrect's two flavours, the
`<= 0` rule, the text format - independently of the device code, which makes the restatement a trustworthy source of full-precision
expected numbers for tests/test_gpu_makematrix.py."""
import numpy as np
import pytest

import golden_util as G
import makematrix_py as M

CASES = ["mm_nt_130x75", "mm_nt_130x75_double", "mm_nt_130x75_raw", "mm_aa_130x75", "mm_aa_130x75_double", "mm_aa_130x75_raw",
         "mm_nt_65x17", "mm_nt_2x1", "mm_aa_70x33"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_text(name):
    d = G.load(name)
    codes, names, n_codes, dt, rawdist = M.fixture_case(d)
    assert len(names) == len(codes)
    got = M.text(names, M.fixture_matrix(d))
    want = bytes(d["text"])
    assert got == want, "first differing byte %d" % next(k for k, (a, b) in enumerate(zip(got, want)) if a != b)


def entries(text):
    return [tok for line in text.decode().splitlines() for tok in line.split(" ")[1:]]


@pytest.mark.parametrize("name", ["mm_nt_130x75", "mm_aa_130x75"])
def test_precision_is_visible_in_the_text(name):
    """the float and -double-precision runs print different digits: the fixtures must go on pinning the numeric_t roundings"""
    f, d = G.load(name), G.load(name + "_double")
    assert np.array_equal(f["codes"], d["codes"])
    a, b = entries(bytes(f["text"])), entries(bytes(d["text"]))
    assert len(a) == len(b) == len(f["codes"]) ** 2
    assert sum(x != y for x, y in zip(a, b)) >= 1
    # ... and the restatement in the other precision does not print the fixture's text
    assert M.text(M.fixture_case(f)[1], M.fixture_matrix(f, dt=np.float64)) != bytes(f["text"])


def test_planted_rows_of_the_nucleotide_fixture():
    """what the fixture is there for: a row of gaps only prints 3.000000 everywhere (1.000000 raw), its own diagonal included; a
    copied row gives a duplicate row of numbers; two rows without a common column are at 3.000000"""
    d, raw = G.load("mm_nt_130x75"), G.load("mm_nt_130x75_raw")
    codes = d["codes"]
    assert (codes[17] == M.NOCODE).all() and np.array_equal(codes[93], codes[40])
    assert not ((codes[66] != M.NOCODE) & (codes[67] != M.NOCODE)).any()
    rows = [line.split(" ") for line in bytes(d["text"]).decode().splitlines()]
    rows_raw = [line.split(" ") for line in bytes(raw["text"]).decode().splitlines()]
    assert rows[17][1:] == ["3.000000"] * 130 and rows_raw[17][1:] == ["1.000000"] * 130
    assert all(r[1 + 17] == "3.000000" for r in rows)
    assert rows[93][0] == "s93" and rows[93][1:] == rows[40][1:]
    assert rows[66][1 + 67] == rows[67][1 + 66] == "3.000000" and rows_raw[66][1 + 67] == "1.000000"
