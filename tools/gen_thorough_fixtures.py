#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/thor_*.npz from the compiled reference: the thorough-search options `-mlacc N`,
`-slownni`, `-nni N`, `-mlnni N` and `-sprlength N`.

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_thorough_fixtures.py [--jobs N] [file ...]

Alignments: synth.random_descent_codes(n, L, n_codes, mu, gaps, seed).
Per file a list of runs; per run `VeryFastTree <flags> -threads T -seed 1`:
  - with `-nosupport -log`: the tree, for ML runs the TreeLogLk / Rates / SiteCategories lines;
  - as it is: the tree with its supports;
  - the same flags WITHOUT the five options: the control trees.  Asserted per run: the tree differs from the control's ("differs"), its
    topology does ("topology"), its supports alone do ("supports"), or - where the option cannot bite on this alignment - it is the
    control's tree ("equal");
  - at -threads 4: the reference's `NJ` log line is asserted to be the one-thread line, and two runs to print the same bytes.
Keys: codes, n_runs, and per run r<k>_flags, r<k>_threads, r<k>_expect, r<k>_newick, r<k>_newick_support, r<k>_control_newick,
r<k>_control_newick_support, and for ML runs r<k>_loglk / _rates / _ratecat and r<k>_control_loglk / _control_rates / _control_ratecat.
Only data (inputs and expected outputs) is written to tests/golden/."""
import os

import numpy as np

import reference_run as R
from reference_run import GOLDEN, one_run, strip_lengths, synth

WITH_NUMBER = ("-mlacc", "-nni", "-mlnni", "-sprlength")
DIFFERS, TOPOLOGY, EQUAL, SUPPORTS = "differs", "topology", "equal", "supports"

FILES = [
    # name, n_codes, (n, L, mu, gaps, seed), runs = (flags, threads, what the tree does against the control's)
    ("thor_nt_150", 4, (150, 300, 0.10, 0.02, 21), [
        (["-nt", "-mlacc", "2"], 1, DIFFERS),
        (["-nt", "-mlacc", "3"], 1, DIFFERS),
        (["-nt", "-mlacc", "2", "-slownni"], 1, DIFFERS),
        (["-nt", "-spr", "4", "-mlacc", "2", "-slownni"], 1, DIFFERS),
        (["-nt", "-nni", "3"], 1, DIFFERS),
        (["-nt", "-mlnni", "2"], 1, DIFFERS),
        (["-nt", "-mlacc", "2", "-slownni", "-gamma"], 1, DIFFERS),
        (["-nt", "-mlacc", "2", "-slownni"], 4, DIFFERS)]),
    # (one thread only: the reference's four-thread `-gtr -mlacc 2` run of this alignment differs from run to run)
    ("thor_nt_60_gtr", 4, (60, 400, 0.15, 0.05, 22), [
        (["-nt", "-gtr", "-double-precision", "-mlacc", "2"], 1, DIFFERS),
        (["-nt", "-gtr", "-double-precision", "-mlacc", "3"], 1, DIFFERS)]),
    # (one thread only: the reference's four-thread protein runs are unstable)
    ("thor_aa_60_lg", 20, (60, 200, 0.12, 0.02, 23), [
        (["-lg", "-mlacc", "2"], 1, DIFFERS),
        (["-lg", "-slownni"], 1, DIFFERS),
        (["-lg", "-mlacc", "2", "-slownni"], 1, DIFFERS)]),
    ("thor_aa_40_wag_double", 20, (40, 250, 0.15, 0.05, 24), [
        (["-wag", "-double-precision", "-mlacc", "3"], 1, DIFFERS),
        (["-wag", "-double-precision", "-mlnni", "2"], 1, DIFFERS)]),
    ("thor_nt_400_noisy", 4, (400, 100, 0.35, 0.10, 32), [
        (["-nt", "-slownni"], 1, TOPOLOGY),
        (["-nt", "-noml", "-slownni"], 1, TOPOLOGY),
        (["-nt", "-noml", "-sprlength", "2"], 1, TOPOLOGY),
        (["-nt", "-noml", "-nni", "5"], 1, TOPOLOGY),
        (["-nt", "-noml", "-sprlength", "30"], 1, EQUAL)]),   # (the chains of this alignment do not reach 10 steps)
    ("thor_aa_150_noisy", 20, (150, 80, 0.30, 0.05, 33), [
        (["-noml", "-slownni"], 1, TOPOLOGY)]),
    # beyond the register-resident quartet kernels (2 048 nucleotide columns): the workspace kernels
    ("thor_nt_30_x2200", 4, (30, 2200, 0.15, 0.03, 41), [
        (["-nt", "-mlacc", "2"], 1, DIFFERS)]),
    # beyond the 512 columns of the protein quad instance: the whole-column instance
    # (seed 42: the reference does not come back from `-lg -mlacc 2` on that alignment)
    ("thor_aa_24_x600_lg", 20, (24, 600, 0.20, 0.03, 43), [
        (["-lg", "-mlacc", "2"], 1, DIFFERS)]),
    # SPR chains beyond the default's ten steps (`-sprlength 64` prints the tree of 30: no chain of this alignment is longer)
    ("thor_nt_300_chains", 4, (300, 40, 0.70, 0.15, 53), [
        (["-nt", "-noml", "-sprlength", "30"], 1, TOPOLOGY),
        (["-nt", "-noml", "-sprlength", "64"], 1, TOPOLOGY)]),
    # `-mllen` reads the accuracy twice: the SH-like supports always make their second pass (NJ.tcc:6934), the -gtr fit makes N rounds
    # over the rates (NJ.tcc:6462; at N = 2 that is the default's fit, at 3 the lengths move)
    ("thor_nt_150_mllen", 4, (150, 300, 0.10, 0.02, 21), [
        (["-nt", "-nome", "-mllen", "-mlacc", "2"], 1, SUPPORTS),
        (["-nt", "-nome", "-mllen", "-gtr", "-mlacc", "3"], 1, DIFFERS)]),
]


def control_of(flags):
    """the flags without the five options"""
    out, k = [], 0
    while k < len(flags):
        if flags[k] in WITH_NUMBER:
            k += 2
        elif flags[k] == "-slownni":
            k += 1
        else:
            out.append(flags[k])
            k += 1
    return out


def gen_file(tmp, name, nc, shape, runs):
    n, L, mu, gaps, seed = shape
    codes = synth.random_descent_codes(n, L, nc, mu, gaps, seed)
    fa = R.write_fasta(tmp, name, codes, nc)
    out = dict(codes=codes, n_runs=np.int64(len(runs)))
    lines = []
    for k, (flags, threads, expect) in enumerate(runs):
        tag = "%s_r%d" % (name, k)
        got = one_run(tmp, tag, fa, flags, threads)
        ctl = one_run(tmp, tag + "_control", fa, control_of(flags), threads)
        same = bytes(got["newick"]) == bytes(ctl["newick"]) and bytes(got["newick_support"]) == bytes(ctl["newick_support"])
        if expect == EQUAL:
            assert same, tag + ": expected the control's tree"
        elif expect == SUPPORTS:
            assert bytes(got["newick"]) == bytes(ctl["newick"]), tag + ": expected the control's tree but for the supports"
            assert bytes(got["newick_support"]) != bytes(ctl["newick_support"]), tag + ": the options print the control's supports - take another seed"
        else:
            assert bytes(got["newick"]) != bytes(ctl["newick"]), tag + ": the options print the control's tree - take another seed"
            assert bytes(got["newick_support"]) != bytes(ctl["newick_support"]), tag + ": the options print the control's tree - take another seed"
        if expect == TOPOLOGY:
            assert strip_lengths(got["newick"]) != strip_lengths(ctl["newick"]), tag + ": expected another topology than the control's"
        pre = "r%d_" % k
        out[pre + "flags"] = R.as_bytes(" ".join(flags))
        out[pre + "threads"] = np.int64(threads)
        out[pre + "expect"] = R.as_bytes(expect)
        for key, v in got.items():
            out[pre + key] = v
        for key, v in ctl.items():
            out[pre + "control_" + key] = v
        what = "the control's tree" if same else "topology differs from the control" if strip_lengths(got["newick"]) != strip_lengths(ctl["newick"]) else "lengths differ from the control"
        lines.append("    r%d %-52s t%d  %s" % (k, " ".join(flags), threads, what))
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, **out)
    return "%-22s %4d x %4d  %d runs  %6.1f KiB\n%s" % (name, codes.shape[0], codes.shape[1], len(runs), os.path.getsize(dst) / 1024.0, "\n".join(lines))


if __name__ == "__main__":
    R.main(gen_file, FILES)
