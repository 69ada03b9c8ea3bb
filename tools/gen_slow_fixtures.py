#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/slow_*.npz from the compiled reference (`-slow`, exhaustiveNJSearch).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_slow_fixtures.py [--jobs N] [case ...]

Like oracle/gen_fixtures.py's gen_blackbox: `VeryFastTree <flags> -slow -threads 1 -seed 1 -verbose 3 -noml -nome -nosupport
-log ...` for the `Join` lines, the NJ tree and the final tree, a second run without -nosupport for the supported tree; the
keys are those of bb_*.npz.  slow_mllen_* follows gen_mllen (`-nome -mllen`), with the keys of ml_*.npz.  Only data (inputs
and expected outputs) is written to tests/golden/.
"""
import os
import re

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, first_unique, rd, run, synth


def mirror_codes():
    """rows 0-39 are X|Y, rows 40-79 are Y|X: every distance among the first 40 rows is repeated among the last 40"""
    x = synth.random_descent_codes(40, 30, 4, 0.08, 0.0, 51)
    y = synth.random_descent_codes(40, 30, 4, 0.08, 0.0, 52)
    return np.concatenate([np.concatenate([x, y], axis=1), np.concatenate([y, x], axis=1)], axis=0)


CASES = [
    # name, flags, n_codes, alignment
    ("slow_nt_200", ["-nt"], 4, rd(200, 120, 4, 0.05, 0.02, 21)),             # bb_nt_200's alignment
    ("slow_nt_600", ["-nt"], 4, rd(600, 100, 4, 0.04, 0.02, 22)),
    ("slow_nt_1500", ["-nt"], 4, rd(1500, 80, 4, 0.03, 0.01, 23)),            # out-profile resets happen
    ("slow_nt_300_double", ["-nt", "-double-precision"], 4, rd(300, 90, 4, 0.05, 0.03, 24)),
    ("slow_aa_300", [], 20, rd(300, 80, 20, 0.10, 0.03, 25)),                 # codeDist: the orientation of profileDist
    ("slow_nt_mirror", ["-nt"], 4, mirror_codes),                            # exact ties
    ("slow_nt_mirror_double", ["-nt", "-double-precision"], 4, mirror_codes),
    ("slow_nt_5", ["-nt"], 4, rd(5, 40, 4, 0.2, 0.0, 27)),                    # bb_nt_5's alignment: two joins
    ("slow_nt_4", ["-nt"], 4, lambda: synth.random_descent_codes(5, 40, 4, 0.2, 0.0, 27)[:4]),   # one join
    # one past a 64-column chunk of a matrix row / one past four such chunks (256 columns)
    ("slow_nt_65", ["-nt"], 4, lambda: first_unique(synth.random_descent_codes(90, 40, 4, 0.10, 0.02, 61), 65)),
    ("slow_nt_257", ["-nt"], 4, lambda: first_unique(synth.random_descent_codes(330, 40, 4, 0.10, 0.02, 62), 257)),
]
MLLEN_CASES = [
    ("slow_mllen_nt_200", ["-nt", "-nocat"], 4, rd(200, 120, 4, 0.05, 0.02, 21)),   # ml_nt_200's flags plus -slow
]


def gen_case(tmp, name, flags, nc, make):
    codes = make()
    fa = R.write_fasta(tmp, name, codes, nc)
    log = os.path.join(tmp, name + ".log")
    res = run([REFBIN] + flags + ["-slow", "-threads", "1", "-seed", "1", "-verbose", "3", "-noml", "-nome", "-nosupport", "-log", log, fa])
    text = R.read_log(log) + "\n" + res.stderr.decode(errors="replace")
    joins, seen = [], set()
    for m in re.finditer(r"^Join\t(\d+)\t(\d+)\t(\S+)\tlambda\t\S+\tselfw\t\S+\t\S+\tnew\t(\d+)", text, re.M):
        if int(m.group(4)) not in seen:   # log and stderr may both carry the lines
            seen.add(int(m.group(4)))
            joins.append((int(m.group(1)), int(m.group(2)), int(m.group(4)), float(m.group(3))))
    assert joins, "no Join lines for " + name
    res2 = run([REFBIN] + flags + ["-slow", "-threads", "1", "-seed", "1", "-noml", "-nome", fa])
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, joins=np.array([j[:3] for j in joins], dtype=np.int64),
                        join_criterion=np.array([j[3] for j in joins], dtype=np.float64),
                        newick=R.as_bytes(res.stdout), nj_newick=R.as_bytes(R.nj_line(text)), newick_support=R.as_bytes(res2.stdout),
                        flags=R.as_bytes(" ".join(flags + ["-slow"])))
    return "%-24s %5d joins  %7.1f KiB" % (name, len(joins), os.path.getsize(dst) / 1024.0)


def gen_mllen_case(tmp, name, flags, nc, make):
    codes = make()
    got = R.one_run(tmp, name, R.write_fasta(tmp, name, codes, nc), flags + ["-slow", "-nome", "-mllen"], 1)
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, loglk=got["loglk"], newick=got["newick"], newick_support=got["newick_support"], rates=got["rates"],
                        ratecat=got["ratecat"], flags=R.as_bytes(" ".join(flags + ["-slow"])))
    return "%-24s %2d rounds  final logLk %.4f  %7.1f KiB" % (name, len(got["loglk"]), got["loglk"][-1], os.path.getsize(dst) / 1024.0)


def gen_any(tmp, name, *case):
    return (gen_mllen_case if name.startswith("slow_mllen_") else gen_case)(tmp, name, *case)


if __name__ == "__main__":
    R.main(gen_any, CASES + MLLEN_CASES)
