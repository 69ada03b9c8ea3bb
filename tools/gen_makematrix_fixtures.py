#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/mm_*.npz from the compiled reference (`-makematrix`, printDistances).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_makematrix_fixtures.py [case ...]

`VeryFastTree <flags> -makematrix -threads 1 in.fasta`: the standard output is the matrix.  Keys: codes (the whole alignment, every
row), names (joined with newlines), flags, text (the reference's standard output, bytes).  Only data is written to tests/golden/.
Alignments are synth.random_descent_codes plus planted rows; each `_double` case must differ from its float sibling in at least one
printed entry (the numeric_t roundings of seqDist and logCorrect are visible in the text), or the pair would pin nothing.
"""
import os
import sys
import tempfile

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, run, synth

NOCODE = synth.NOCODE


def nt_130x75():
    """two full 64-lane tiles and a partial one; four 16-column chunks and a partial one; planted: a row of gaps only, a row copied
    from another, two rows whose present columns do not overlap"""
    codes = synth.random_descent_codes(130, 75, 4, 0.15, 0.05, 71)
    codes[17] = NOCODE          # gaps only
    codes[93] = codes[40]       # a duplicate sequence: a duplicate row, not uniquified
    codes[66, 37:] = NOCODE     # present in columns 0..36 only
    codes[67, :37] = NOCODE     # present in columns 37..74 only
    return codes


def aa_130x75():
    codes = synth.random_descent_codes(130, 75, 20, 0.20, 0.05, 72)
    codes[5] = NOCODE
    codes[128] = codes[2]
    return codes


CASES = [
    # name, flags, n_codes, alignment
    ("mm_nt_130x75", ["-nt"], 4, nt_130x75),
    ("mm_nt_130x75_double", ["-nt", "-double-precision"], 4, nt_130x75),
    ("mm_nt_130x75_raw", ["-nt", "-rawdist"], 4, nt_130x75),
    ("mm_aa_130x75", [], 20, aa_130x75),
    ("mm_aa_130x75_double", ["-double-precision"], 20, aa_130x75),
    ("mm_aa_130x75_raw", ["-rawdist"], 20, aa_130x75),
    ("mm_nt_65x17", ["-nt"], 4, lambda: synth.random_descent_codes(65, 17, 4, 0.15, 0.05, 73)),   # one past a tile, one past a chunk
    ("mm_nt_2x1", ["-nt"], 4, lambda: np.array([[0], [2]], np.uint8)),                              # smallest case
    ("mm_aa_70x33", [], 20, lambda: synth.random_descent_codes(70, 33, 20, 0.20, 0.05, 74)),
]


def gen_case(tmp, name, flags, nc, make):
    codes = np.ascontiguousarray(make(), np.uint8)
    names = ["s%d" % k for k in range(len(codes))]   # what synth.codes_to_fasta writes
    text = run([REFBIN] + flags + ["-makematrix", "-threads", "1", R.write_fasta(tmp, name, codes, nc)]).stdout
    assert text.count(b"\n") == len(codes), "%s: %d lines for %d sequences" % (name, text.count(b"\n"), len(codes))
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, names=R.as_bytes("\n".join(names)), flags=R.as_bytes(" ".join(flags + ["-makematrix"])), text=R.as_bytes(text))
    return text, "%-24s %4d x %3d  %7.1f KiB" % (name, codes.shape[0], codes.shape[1], os.path.getsize(dst) / 1024.0)


def entries(text):
    return [tok for line in text.decode().splitlines() for tok in line.split(" ")[1:]]


def main():
    want = sys.argv[1:]
    assert os.path.exists(REFBIN), "build the reference first: make -C oracle ref"
    texts = {}
    with tempfile.TemporaryDirectory() as tmp:
        for c in CASES:
            if want and c[0] not in want:
                continue
            texts[c[0]], line = gen_case(tmp, *c)
            print(line, flush=True)
    for name, text in texts.items():
        if name.endswith("_double") and name[:-len("_double")] in texts:
            a, b = entries(texts[name[:-len("_double")]]), entries(text)
            differ = sum(x != y for x, y in zip(a, b))
            assert len(a) == len(b) and differ >= 1, "%s prints what its float sibling prints" % name
            print("%-24s %d of %d entries differ from the float text" % (name, differ, len(a)))


if __name__ == "__main__":
    main()
