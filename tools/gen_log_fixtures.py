#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/log_*.npz from the compiled reference's `-log FILE`.

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_log_fixtures.py [--jobs N] [case ...]

Per case two runs of `VeryFastTree <flags> -seed 1 -threads T [-intree T.nwk] -log L`.  Stored: codes, flags (what
veryfasttree_amd/refflags.py translates; the threads and the start tree apart, as in the other fixtures), threads, intree where there is
one, `log` = the in-scope lines of L (veryfasttree_amd/stagelog.py) joined by newlines, the clock fields masked with `#`, and `newick` =
the tree the run printed (with its supports).  A case whose two runs do not print the same in-scope lines is dropped and named.  Only
data - inputs and recorded outputs - is written to tests/golden/."""
import os

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, first_unique, rd, run, synth
from gen_intree_fixtures import random_tree
from veryfasttree_amd import stagelog


def with_duplicates(n, L, nc, mu, gap, seed, copies):
    """n unique rows, then a copy of each row of `copies` - `Unique: n/(n + len(copies))` in the summary"""
    def make():
        u = first_unique(synth.random_descent_codes(n + 20, L, nc, mu, gap, seed), n)
        return np.concatenate([u] + [u[k:k + 1] for k in copies], axis=0)
    return make


CASES = [
    # name, flags, n_codes, threads, alignment, start tree or None
    ("log_nt_default", ["-nt"], 4, 1, with_duplicates(60, 150, 4, 0.08, 0.03, 301, (3, 3, 17)), None),
    ("log_nt_gtr_gamma", ["-nt", "-gtr", "-gamma"], 4, 1, rd(40, 150, 4, 0.08, 0.03, 302), None),
    ("log_nt_double_gtr", ["-nt", "-double-precision", "-gtr"], 4, 1, rd(48, 120, 4, 0.07, 0.02, 303), None),
    ("log_nt_noml", ["-nt", "-noml"], 4, 1, rd(100, 100, 4, 0.06, 0.03, 304), None),
    ("log_nt_noml_nome", ["-nt", "-noml", "-nome"], 4, 1, rd(200, 100, 4, 0.05, 0.02, 305), None),
    ("log_nt_mllen_nocat", ["-nt", "-nome", "-mllen", "-nocat"], 4, 1, rd(64, 120, 4, 0.08, 0.02, 306), None),
    ("log_nt_mllen_cat5", ["-nt", "-nome", "-mllen", "-cat", "5"], 4, 1, rd(64, 120, 4, 0.08, 0.02, 307), None),
    ("log_aa_lg_gamma", ["-lg", "-gamma"], 20, 1, rd(32, 100, 20, 0.10, 0.03, 308), None),
    ("log_aa_wag_double", ["-wag", "-double-precision"], 20, 1, rd(32, 100, 20, 0.10, 0.03, 309), None),
    ("log_aa_jtt_approxml", ["-approxml"], 20, 1, rd(40, 100, 20, 0.12, 0.03, 310), None),   # (threaded -approxml does not repeat: one thread)
    ("log_nt_thorough", ["-nt", "-spr", "4", "-mlacc", "2", "-slownni"], 4, 1, rd(48, 150, 4, 0.08, 0.03, 311), None),
    ("log_nt_t4", ["-nt"], 4, 4, rd(120, 150, 4, 0.07, 0.02, 312), None),
    ("log_nt_noml_t4", ["-nt", "-noml"], 4, 4, rd(120, 150, 4, 0.07, 0.02, 317), None),
    ("log_nt_nosupport", ["-nt", "-nosupport"], 4, 1, rd(48, 120, 4, 0.08, 0.02, 318), None),   # (the splits are tested for the summary alone)
    ("log_nt_fastest_nosupport", ["-nt", "-fastest", "-nosupport"], 4, 1, rd(48, 120, 4, 0.08, 0.02, 319), None),   # (and here they are not)
    ("log_nt_intree", ["-nt"], 4, 1, rd(50, 120, 4, 0.08, 0.02, 313), random_tree(50, 314, False)),
    ("log_nt_slow_mllen", ["-nt", "-slow", "-nome", "-mllen"], 4, 1, rd(40, 120, 4, 0.08, 0.02, 315), None),
    ("log_nt_noml_nome_pseudo", ["-nt", "-noml", "-nome", "-pseudo"], 4, 1, rd(48, 120, 4, 0.10, 0.15, 320), None),   # (the ME bad splits under pseudocounts)
    ("log_nt_pseudo", ["-nt", "-pseudo"], 4, 1, rd(48, 120, 4, 0.10, 0.15, 316), None),
]


def gen_case(tmp, name, flags, nc, threads, make, start):
    codes = make()
    fa = R.write_fasta(tmp, name, codes, nc)
    cmd = [REFBIN] + flags + ["-seed", "1", "-threads", str(threads)]
    if start:
        nwk = os.path.join(tmp, name + ".nwk")
        with open(nwk, "w") as fh:
            fh.write(start)
        cmd += ["-intree", nwk]
    runs = []
    for k in (1, 2):
        log = os.path.join(tmp, "%s_%d.log" % (name, k))
        res = run(cmd + ["-log", log, fa])
        runs.append((stagelog.masked_lines(R.read_log(log)), res.stdout))
    why = stagelog.first_difference(runs[0][0], runs[1][0])
    if why or runs[0][1] != runs[1][1]:
        return "%-24s DROPPED: two runs of the reference differ (%s)" % (name, why or "the printed tree")
    lines = runs[0][0]
    assert lines and lines[-1] == "TreeCompleted", name + ": the log does not end with TreeCompleted"
    out = dict(codes=codes, flags=R.as_bytes(" ".join(flags)), threads=np.int64(threads), log=R.as_bytes("\n".join(lines)), newick=R.as_bytes(runs[0][1]))
    if start:
        out["intree"] = R.as_bytes(start)
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, **out)
    return "%-24s %4d rows x %4d  %4d lines  %7.1f KiB" % (name, codes.shape[0], codes.shape[1], len(lines), os.path.getsize(dst) / 1024.0)


if __name__ == "__main__":
    R.main(gen_case, CASES)
