#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/lsup_*.npz from the compiled reference: local-bootstrap supports
(splitSupport) on alignments longer than the 1 706 columns k_split_support holds in LDS.

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`); CPU only:

    python tools/gen_longsupport_fixtures.py [--jobs N] [case ...]

Per case one run of `VeryFastTree <flags> -threads 1 -log LOG`: its standard output is the final tree (ME lengths, local
supports), the log's `NJ` and `ME_Lengths` lines are the trees before the supports stage.  The shapes are the smallest at
which each number of pairs per pass of k_split_support_long and each boundary between them is reached.
Only data (inputs and expected outputs) is written to tests/golden/: codes, flags, newick_support, nj_newick, me_lengths.
"""
import os
import re

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, first_unique, run, synth

NOCODE = 127
MIN_DISTINCT_SUPPORTS = 3


def rd(n, L, nc, mu, gap, seed):
    return lambda: first_unique(synth.random_descent_codes(2 * n, L, nc, mu, gap, seed), n)


def gappy_codes():
    """14 x 2 400: s0-s2 cover only the first 300 columns, s3-s5 only the last 300 - quartets with pairs that share no
    column (totw <= 0.01 -> the distance 3.0 of splitSupport) occur"""
    codes = rd(14, 2400, 4, 0.08, 0.01, 47)().copy()
    codes[0:3, 300:] = NOCODE
    codes[3:6, :2100] = NOCODE
    return codes


CASES = [
    # name, reference flags, n_codes, alignment
    ("lsup_nt_16x1707", ["-nt", "-noml", "-nome"], 4, rd(16, 1707, 4, 0.015, 0.02, 41)),                      # 3 pairs per pass, first length
    ("lsup_nt_16x1707_boot100", ["-nt", "-noml", "-nome", "-boot", "100"], 4, rd(16, 1707, 4, 0.015, 0.02, 41)),   # the same alignment
    ("lsup_nt_12x3414_double", ["-nt", "-noml", "-nome", "-double-precision"], 4, rd(12, 3414, 4, 0.01, 0.02, 42)),   # 2 pairs, first length
    ("lsup_nt_12x5121_me", ["-nt", "-noml"], 4, rd(12, 5121, 4, 0.008, 0.02, 43)),                             # 1 pair, after ME NNIs and SPRs
    ("lsup_nt_8x10224", ["-nt", "-noml", "-nome"], 4, rd(8, 10224, 4, 0.004, 0.02, 44)),                       # the longest the NJ phase runs
    ("lsup_aa_12x2000", ["-noml", "-nome"], 20, rd(12, 2000, 20, 0.02, 0.02, 45)),                             # BLOSUM45 pieces, scoredist
    ("lsup_aa_10x3500_double", ["-noml", "-nome", "-double-precision"], 20, rd(10, 3500, 20, 0.012, 0.02, 46)),   # 2 pairs, 20 states, double
    ("lsup_nt_14x2400_gappy", ["-nt", "-noml", "-nome"], 4, gappy_codes),
]


def supports_of(tree):
    return re.findall(r"\)([0-9.]+):", tree)


def gen_case(tmp, name, flags, nc, make):
    codes = make()
    assert len({r.tobytes() for r in codes}) == len(codes), name + ": duplicate rows"
    fa = R.write_fasta(tmp, name, codes, nc)
    log = os.path.join(tmp, name + ".log")
    res = run([REFBIN] + flags + ["-threads", "1", "-log", log, fa])
    ltext = R.read_log(log)
    tree = res.stdout.decode()
    sup = supports_of(tree)
    assert len(sup) == len(codes) - 3, "%s: %d supports for %d sequences" % (name, len(sup), len(codes))
    distinct = sorted(set(sup))
    assert len(distinct) >= MIN_DISTINCT_SUPPORTS, "%s: supports %s - choose another mutation rate" % (name, distinct)
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, flags=R.as_bytes(" ".join(flags)), newick_support=R.as_bytes(res.stdout), nj_newick=R.as_bytes(R.nj_line(ltext)),
                        me_lengths=R.as_bytes(R.nj_line(ltext, "ME_Lengths")), n_distinct_supports=np.int64(len(distinct)))
    assert os.path.getsize(dst) < (1 << 20), name + ": larger than a committed file may be"
    return "%-28s %3d x %5d  %2d distinct supports %s  %6.1f KiB" % (name, codes.shape[0], codes.shape[1], len(distinct), " ".join(distinct), os.path.getsize(dst) / 1024.0)


if __name__ == "__main__":
    R.main(gen_case, CASES)
