#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/approx_aa_*.npz from the compiled reference (`-approxml`, the near-constant
posteriors of posteriorProfile, NJ.tcc:2390-2421).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_approxml_fixtures.py [--jobs N] [case ...]

Per case `VeryFastTree <flags> -approxml -threads 1 -seed 1` through reference_run.one_run (the keys of the full_* / ml_* files: codes,
flags, newick, newick_support, loglk, rates, ratecat) and the same command without -approxml for `control_newick`.  One thread only: the
reference's own runs with the flag at several threads do not repeat.  The generator insists that two runs with the flag print the same
bytes and that they are not the control's; and, once, that under -nt the flag changes nothing.  Only data (inputs and expected outputs)
is written to tests/golden/."""
import os

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, rd, run

CASES = [
    # name, flags, alignment
    ("approx_aa_jtt_60", [], rd(60, 80, 20, 0.10, 0.03, 11)),
    ("approx_aa_lg_120", ["-lg"], rd(120, 150, 20, 0.05, 0.02, 12)),
    ("approx_aa_wag_100_double", ["-wag", "-double-precision"], rd(100, 300, 20, 0.03, 0.02, 13)),
    ("approx_aa_wag_100_double_mllen", ["-wag", "-double-precision", "-nome", "-mllen"], rd(100, 300, 20, 0.03, 0.02, 13)),
    ("approx_aa_lg_40_double_gamma", ["-lg", "-double-precision", "-gamma"], rd(40, 600, 20, 0.15, 0.05, 14)),   # beyond the quad kernels' 512 columns
    ("approx_aa_lg_12_long", ["-lg"], rd(12, 2200, 20, 0.10, 0.03, 16)),                                          # the workspace kernels
    ("approx_aa_lg_60_thorough", ["-lg", "-mlacc", "2", "-slownni"], rd(60, 100, 20, 0.10, 0.03, 17)),
]


def check_nt_is_inert(tmp):
    """-nt -approxml prints what -nt prints"""
    fa = R.write_fasta(tmp, "approx_nt", rd(50, 100, 4, 0.08, 0.02, 18)(), 4)
    base = [REFBIN, "-nt", "-threads", "1", "-seed", "1"]
    assert run(base + ["-approxml", fa]).stdout == run(base + [fa]).stdout, "-nt -approxml differs from -nt"


def gen_case(tmp, name, flags, make):
    if name == CASES[0][0]:
        check_nt_is_inert(tmp)
    codes = make()
    fa = R.write_fasta(tmp, name, codes, 20)
    got = R.one_run(tmp, name, fa, flags + ["-approxml"], 1)
    again = run([REFBIN] + flags + ["-approxml", "-threads", "1", "-seed", "1", fa]).stdout
    assert again == bytes(got["newick_support"]), name + ": two runs with -approxml print different trees"
    control = run([REFBIN] + flags + ["-threads", "1", "-seed", "1", "-nosupport", fa]).stdout
    assert control != bytes(got["newick"]), name + ": -approxml changes nothing here"
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, codes=codes, loglk=got["loglk"], newick=got["newick"], newick_support=got["newick_support"], rates=got["rates"],
                        ratecat=got["ratecat"], control_newick=R.as_bytes(control), flags=R.as_bytes(" ".join(flags + ["-approxml"])))
    assert os.path.getsize(dst) < (1 << 20), name
    return "%-32s %2d TreeLogLk lines  final logLk %.4f  %7.1f KiB" % (name, len(got["loglk"]), got["loglk"][-1], os.path.getsize(dst) / 1024.0)


if __name__ == "__main__":
    R.main(gen_case, CASES)
