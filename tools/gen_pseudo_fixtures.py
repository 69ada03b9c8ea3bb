#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/pseudo_*.npz from the compiled reference (`-pseudo [weight]`, correctedPairDistances).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_pseudo_fixtures.py [--jobs N] [file ...]

Alignments in which many sequences share few or no columns - what the option is for:
  fragments  random_descent_codes(n, L, nc, 0.08, 0.02, seed), then every row keeps one window of int(L * keep) columns (its start drawn
             from PCG64(seed + 1000), row by row) and is a gap everywhere else;
  ladder     8 sequences on 72 columns: sequence k covers columns [8k, 8k + 16) of a copy of one random base sequence with 20 % of the
             sites redrawn - neighbours share 8 columns, every other pair none.
Per file a list of runs; per run `VeryFastTree <flags> -threads T -seed 1`:
  - with `-nosupport -log`: the tree, for ML runs the TreeLogLk / Rates / SiteCategories lines;
  - as it is: the tree with its supports;
  - the same flags WITHOUT -pseudo: the control trees (asserted to differ from the -pseudo ones);
  - at -threads 4: the reference's `NJ` log line is asserted to be the one-thread line, and two runs to print the same bytes.
Keys: codes, n_runs, and per run r<k>_flags (with -pseudo), r<k>_threads, r<k>_pseudo, r<k>_newick, r<k>_newick_support, r<k>_control_newick,
r<k>_control_newick_support, r<k>_intree (when the run starts from a tree), and for ML runs r<k>_loglk / _rates / _ratecat and
r<k>_control_loglk / _control_rates / _control_ratecat.  Only data (inputs and expected outputs) is written to tests/golden/."""
import os
import re

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, run, synth


def fragments(n, L, nc, seed, keep):
    def make():
        codes = synth.random_descent_codes(n, L, nc, 0.08, 0.02, seed)
        rng = np.random.Generator(np.random.PCG64(seed + 1000))
        w = int(L * keep)
        for k in range(n):
            s = int(rng.integers(0, L - w + 1))
            codes[k, :s] = synth.NOCODE
            codes[k, s + w:] = synth.NOCODE
        return codes
    return make


LADDER_SEED = 5


def ladder():
    rng = np.random.Generator(np.random.PCG64(LADDER_SEED))
    base = rng.integers(0, 4, 72)
    codes = np.full((8, 72), synth.NOCODE, np.uint8)
    for k in range(8):
        copy = base.copy()
        redraw = rng.random(72) < 0.2
        copy[redraw] = rng.integers(0, 4, int(redraw.sum()))
        codes[k, 8 * k:8 * k + 16] = copy[8 * k:8 * k + 16]
    return codes


INTREE = "INTREE"   # placeholder in a run's flags: `-intree T`, T = the reference's `-noml -nome -nosupport` tree of the alignment

FILES = [
    # name, n_codes, alignment, runs = (flags with -pseudo [W], threads)
    ("pseudo_nt_8_ladder", 4, ladder, [
        (["-nt", "-pseudo", "-noml", "-nome", "-nosupport"], 1),
        (["-nt", "-pseudo", "-noml"], 1),
        (["-nt", "-pseudo"], 1)]),
    ("pseudo_nt_60_frag", 4, fragments(60, 120, 4, 11, 0.35), [
        (["-nt", "-noml", "-pseudo"], 1),
        (["-nt", "-noml", "-pseudo", "0.5"], 1),
        (["-nt", "-noml", "-pseudo", "3"], 1),
        (["-nt", "-pseudo"], 1),
        (["-nt", "-slow", "-noml", "-nome", "-pseudo"], 1),
        (["-nt", "-noml", "-pseudo", "2", INTREE], 1),
        (["-nt", "-noml", "-pseudo"], 4)]),
    ("pseudo_nt_200_frag", 4, fragments(200, 200, 4, 12, 0.30), [
        (["-nt", "-pseudo"], 1),
        (["-nt", "-pseudo"], 4),
        (["-nt", "-gtr", "-double-precision", "-pseudo"], 1)]),
    # (one thread only: the reference's four-thread runs of this alignment differ from run to run)
    ("pseudo_aa_80_frag", 20, fragments(80, 100, 20, 13, 0.35), [
        (["-pseudo"], 1),
        (["-lg", "-double-precision", "-pseudo"], 1)]),
]


def without_pseudo(flags):
    """the flags of the control run, and the weight the -pseudo run asked for"""
    k = flags.index("-pseudo")
    try:
        return flags[:k] + flags[k + 2:], float(flags[k + 1])
    except (IndexError, ValueError):
        return flags[:k] + flags[k + 1:], 1.0


def one_run(tmp, tag, fa, flags, threads, intree):
    return R.one_run(tmp, tag, fa, [f for f in flags if f != INTREE], threads, intree if INTREE in flags else None)


def gen_file(tmp, name, nc, make, runs):
    codes = make()
    fa = R.write_fasta(tmp, name, codes, nc)
    out = dict(codes=codes, n_runs=np.int64(len(runs)))
    intree = os.path.join(tmp, name + ".nwk")
    if any(INTREE in flags for flags, _ in runs):
        start = run([REFBIN, "-nt", "-noml", "-nome", "-nosupport", "-threads", "1", "-seed", "1", fa]).stdout
        with open(intree, "wb") as fh:
            fh.write(start)
    lines = []
    for k, (flags, threads) in enumerate(runs):
        tag = "%s_r%d" % (name, k)
        control, weight = without_pseudo(flags)
        got = one_run(tmp, tag, fa, flags, threads, intree)
        ctl = one_run(tmp, tag + "_control", fa, control, threads, intree)
        assert bytes(got["newick"]) != bytes(ctl["newick"]), tag + ": -pseudo prints the control's tree"
        assert "-nosupport" in flags or bytes(got["newick_support"]) != bytes(ctl["newick_support"]), tag + ": -pseudo prints the control's tree"
        pre = "r%d_" % k
        out[pre + "flags"] = R.as_bytes(" ".join(f for f in flags if f != INTREE))
        out[pre + "threads"] = np.int64(threads)
        out[pre + "pseudo"] = np.float64(weight)
        if INTREE in flags:
            out[pre + "intree"] = R.as_bytes(open(intree, "rb").read())
        for key, v in got.items():
            out[pre + key] = v
        for key, v in ctl.items():
            out[pre + "control_" + key] = v
        strip = lambda t: re.sub(rb":[0-9.eE+-]+", b":", bytes(t))
        lines.append("    r%d %-44s t%d  %s" % (k, " ".join(flags), threads, "topology differs from the control" if strip(got["newick"]) != strip(ctl["newick"]) else "lengths differ from the control"))
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, **out)
    return "%-22s %4d x %4d  %d runs  %6.1f KiB\n%s" % (name, codes.shape[0], codes.shape[1], len(runs), os.path.getsize(dst) / 1024.0, "\n".join(lines))


if __name__ == "__main__":
    R.main(gen_file, FILES)
