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
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veryfasttree_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "VeryFastTree")
NOCODE = 127
MIN_DISTINCT_SUPPORTS = 3


def rd(n, L, nc, mu, gap, seed):
    return lambda: first_unique(synth.random_descent_codes(2 * n, L, nc, mu, gap, seed), n)


def first_unique(codes, k):
    seen, rows = set(), []
    for row in codes:
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            rows.append(row)
        if len(rows) == k:
            return np.stack(rows)
    raise AssertionError("fewer than %d unique rows" % k)


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


def run(cmd):
    env = dict(os.environ, OMP_WAIT_POLICY="passive")
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def supports_of(tree):
    return re.findall(r"\)([0-9.]+):", tree)


def gen_case(tmp, name, flags, nc, make):
    codes = make()
    assert len({r.tobytes() for r in codes}) == len(codes), name + ": duplicate rows"
    fa = os.path.join(tmp, name + ".fa")
    synth.codes_to_fasta(codes, fa, synth.ALPHABET_AA if nc == 20 else synth.ALPHABET_NT)
    log = os.path.join(tmp, name + ".log")
    res = run([REFBIN] + flags + ["-threads", "1", "-log", log, fa])
    ltext = open(log, errors="replace").read()
    mnj = re.search(r"^NJ\t(\(.*;)\s*$", ltext, re.M)
    mme = re.search(r"^ME_Lengths\t(\(.*;)\s*$", ltext, re.M)
    assert mnj and mme, name + ": no NJ / ME_Lengths line"
    tree = res.stdout.decode()
    sup = supports_of(tree)
    assert len(sup) == len(codes) - 3, "%s: %d supports for %d sequences" % (name, len(sup), len(codes))
    distinct = sorted(set(sup))
    assert len(distinct) >= MIN_DISTINCT_SUPPORTS, "%s: supports %s - choose another mutation rate" % (name, distinct)
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, flags=np.frombuffer(" ".join(flags).encode(), dtype=np.uint8),
                        newick_support=np.frombuffer(res.stdout, dtype=np.uint8), nj_newick=np.frombuffer(mnj.group(1).encode(), dtype=np.uint8),
                        me_lengths=np.frombuffer(mme.group(1).encode(), dtype=np.uint8), n_distinct_supports=np.int64(len(distinct)))
    assert os.path.getsize(dst) < (1 << 20), name + ": larger than a committed file may be"
    return "%-28s %3d x %5d  %2d distinct supports %s  %6.1f KiB" % (name, codes.shape[0], codes.shape[1], len(distinct), " ".join(distinct), os.path.getsize(dst) / 1024.0)


def main():
    args = sys.argv[1:]
    jobs = 4
    if "--jobs" in args:
        k = args.index("--jobs")
        jobs = int(args[k + 1])
        del args[k:k + 2]
    assert os.path.exists(REFBIN), "build the reference first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as pool:
        futs = [pool.submit(gen_case, tmp, *c) for c in CASES if not args or c[0] in args]
        for f in futs:
            print(f.result(), flush=True)


if __name__ == "__main__":
    main()
