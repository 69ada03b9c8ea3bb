#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/rawdist_*.npz and trans_*.npz from the compiled reference: `-rawdist` for a tree (no
log correction in the minimum-evolution stages) and `-trans FILE` (a rate matrix of the user's for the ML stage).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_distopt_fixtures.py [--jobs N] [file ...]

Per file a list of runs; per run `VeryFastTree <flags> -threads T -seed 1`, through reference_run.one_run:
  - with `-nosupport -log`: the tree, for ML runs the TreeLogLk / Rates / SiteCategories lines; as it is: the tree with its supports;
  - the same flags WITHOUT the option: the control (r<k>_control_*).
Asserted for every run: a second run of the reference prints the same bytes, and the run differs from its control.
The matrix of the trans_* files is this generator's own: symmetric exchangeabilities drawn from (0.05, 2), Dirichlet(8) frequencies
(PCG64(MATRIX_SEED)), rate(i, j) = s_ij * pi_i, columns summing to 0, normalised to one substitution per unit time, written with
%.12g in the layout readAATransitionMatrix reads.
`-trans` at four threads did not repeat in the reference (like -approxml): no such run is recorded.
Keys: codes, n_runs, trans_text (trans_* only: the matrix file's bytes), per run r<k>_flags (with the option; `-trans model.txt` names no
file that exists), r<k>_threads, r<k>_newick, r<k>_newick_support, r<k>_intree (a run that starts from a tree), for ML runs r<k>_loglk /
_rates / _ratecat, and r<k>_control_<the same>.  Only data (inputs and expected outputs) is written to tests/golden/."""
import os
import re

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, run

AA = "ARNDCQEGHILKMFPSTWYV"
MATRIX_SEED = 20
TRANS_NAME = "model.txt"
INTREE = "INTREE"   # placeholder in a run's flags: `-intree T`, T = the reference's `-noml -nome -nosupport` tree of the alignment


def random_model(seed=MATRIX_SEED):
    """(matrix[20, 20], stat[20]) of a reversible model: rate(i, j) = s_ij * pi_i off the diagonal"""
    rng = np.random.Generator(np.random.PCG64(seed))
    s = rng.uniform(0.05, 2.0, (20, 20))
    s = np.triu(s, 1) + np.triu(s, 1).T
    pi = rng.dirichlet(np.full(20, 8.0))
    m = s * pi[:, None]
    m[np.arange(20), np.arange(20)] = -m.sum(0)
    m /= -(pi * np.diag(m)).sum()
    return m, pi


def model_text(matrix, stat, fmt="%.12g"):
    lines = ["\t".join(AA) + "\t*"]
    for i in range(20):
        lines.append("\t".join([AA[i]] + [fmt % matrix[i, j] for j in range(20)] + [fmt % stat[i]]))
    return ("\n".join(lines) + "\n").encode()


NT60 = R.rd(60, 80, 4, 0.12, 0.03, 91)
AA40 = R.rd(40, 60, 20, 0.2, 0.05, 92)

FILES = [
    # name, n_codes, alignment, the option, runs = (flags with the option, threads)
    ("rawdist_nt_60", 4, NT60, "-rawdist", [
        (["-nt", "-rawdist"], 1),
        (["-nt", "-noml", "-rawdist"], 1),
        (["-nt", "-noml", "-nome", "-rawdist"], 1),
        (["-nt", "-nome", "-mllen", "-rawdist"], 1),
        (["-nt", "-noml", "-pseudo", "-rawdist"], 1),
        (["-nt", "-double-precision", "-gtr", "-rawdist"], 1),
        (["-nt", "-rawdist"], 4),
        (["-nt", "-noml", "-rawdist"], 4),
        (["-nt", "-slow", "-noml", "-nome", "-rawdist"], 1),
        (["-nt", "-noml", "-nome", "-rawdist", INTREE], 1)]),
    ("rawdist_aa_40", 20, AA40, "-rawdist", [
        (["-rawdist"], 1),
        (["-noml", "-rawdist"], 1),
        (["-noml", "-nome", "-rawdist"], 1),
        (["-lg", "-double-precision", "-rawdist"], 1)]),
    # one column beyond the single-kernel supports: the pass kernel takes the raw flavour
    ("rawdist_nt_16x1707", 4, R.rd(16, 1707, 4, 0.1, 0.02, 93), "-rawdist", [
        (["-nt", "-noml", "-nome", "-rawdist"], 1)]),
    ("trans_aa_40", 20, AA40, "-trans", [
        (["-trans", TRANS_NAME], 1),
        (["-nome", "-mllen", "-trans", TRANS_NAME], 1),
        (["-double-precision", "-gamma", "-trans", TRANS_NAME], 1),
        (["-approxml", "-trans", TRANS_NAME], 1),
        (["-mlacc", "2", "-slownni", "-trans", TRANS_NAME], 1),
        (["-nocat", "-trans", TRANS_NAME], 1)]),
    # beyond 2 048 columns: the ML workspace kernels
    ("trans_aa_12x2200", 20, R.rd(12, 2200, 20, 0.2, 0.02, 94), "-trans", [
        (["-double-precision", "-trans", TRANS_NAME], 1)]),
]


def without(flags, option):
    k = flags.index(option)
    return flags[:k] + flags[k + (2 if option == "-trans" else 1):]


def gen_file(tmp, name, nc, make, option, runs):
    codes = make()
    fa = R.write_fasta(tmp, name, codes, nc)
    out = dict(codes=codes, n_runs=np.int64(len(runs)))
    model = os.path.join(tmp, name + "_" + TRANS_NAME)
    if option == "-trans":
        text = model_text(*random_model())
        with open(model, "wb") as fh:
            fh.write(text)
        out["trans_text"] = R.as_bytes(text)
    intree = os.path.join(tmp, name + ".nwk")
    if any(INTREE in flags for flags, _ in runs):
        start = run([REFBIN, "-nt", "-noml", "-nome", "-nosupport", "-threads", "1", "-seed", "1", fa]).stdout
        with open(intree, "wb") as fh:
            fh.write(start)
    lines = []
    for k, (flags, threads) in enumerate(runs):
        tag = "%s_r%d" % (name, k)
        plain = [f for f in flags if f != INTREE]
        real = [model if f == TRANS_NAME else f for f in plain]
        start = intree if INTREE in flags else None
        got = R.one_run(tmp, tag, fa, real, threads, start)
        again = R.one_run(tmp, tag + "_again", fa, real, threads, start)
        for key in got:
            assert np.array_equal(got[key], again[key]), "%s: two runs of the reference differ in %s" % (tag, key)
        ctl = R.one_run(tmp, tag + "_control", fa, without(real, option), threads, start)
        assert bytes(got["newick"]) != bytes(ctl["newick"]), tag + ": %s prints the control's tree" % option
        assert bytes(got["newick_support"]) != bytes(ctl["newick_support"]), tag + ": %s prints the control's tree" % option
        pre = "r%d_" % k
        out[pre + "flags"] = R.as_bytes(" ".join(plain))
        out[pre + "threads"] = np.int64(threads)
        if start:
            out[pre + "intree"] = R.as_bytes(open(intree, "rb").read())
        for key, v in got.items():
            out[pre + key] = v
        for key, v in ctl.items():
            out[pre + "control_" + key] = v
        strip = lambda t: re.sub(rb":[0-9.eE+-]+", b":", bytes(t))
        lines.append("    r%d %-52s t%d  %s" % (k, " ".join(flags), threads, "topology differs from the control" if strip(got["newick"]) != strip(ctl["newick"]) else "lengths differ from the control"))
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, **out)
    return "%-22s %4d x %4d  %d runs  %6.1f KiB\n%s" % (name, codes.shape[0], codes.shape[1], len(runs), os.path.getsize(dst) / 1024.0, "\n".join(lines))


if __name__ == "__main__":
    R.main(gen_file, FILES)
