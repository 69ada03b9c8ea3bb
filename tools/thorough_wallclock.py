#!/usr/bin/env python3
"""What the accuracy recipe `-spr 4 -mlacc 2 -slownni` costs on one MI355X, next to the reference with the same flags on one thread.

    thorough_wallclock.py [--out profiles/thorough_wallclock.txt] [--limit 900] [--no-reference]

Alignments (the sizes README quotes for the default pipeline): 2 000 x 500 nucleotides (float) and 3 000 x 300 amino acids under
`-lg -double-precision`, synth.random_descent_codes(n, L, n_codes, 0.10, 0.02, seed 51 / 52).  Per alignment, each run in a child process of
its own after a warm-up tree, under a time limit of its own, the first failure ends the tool:
  (a) the default pipeline (me_nni, spr = 2, ml_nni = 20; no supports),
  (b) the recipe (spr = 4, ml_accuracy = 2, slow_nni),
with the seconds per stage of vft_nj_last_stage_seconds; then, where oracle/_ref/VeryFastTree is there, the reference's whole-program
wall clock for `-spr 4 -mlacc 2 -slownni -nosupport -threads 1` where this tool runs (CPU).  No threshold: a measurement."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFBIN = os.path.join(ROOT, "oracle", "_ref", "VeryFastTree")
CASES = {"nt": (2000, 500, 4, 51, np.float32, None, ["-nt"]), "aa": (3000, 300, 20, 52, np.float64, "lg", ["-lg", "-double-precision"])}
RECIPE = dict(spr=4, ml_accuracy=2, slow_nni=True)


def alignment(case):
    from veryfasttree_amd import synth
    n, L, nc, seed = CASES[case][:4]
    return synth.random_descent_codes(n, L, nc, 0.10, 0.02, seed)


def one(case, recipe):
    """one run in this process: prints one JSON line"""
    import zlib
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import nj_newick, last_stage_seconds
    n, L, nc, seed, dt, aa, _ = CASES[case]
    codes = alignment(case)
    names = ["s%d" % k for k in range(n)]
    make = lambda m, cols: HipProfileOps(m, cols, nc, dt, max_nodes=3 * m)
    kw = dict(dtype=dt, me_lengths=True, me_nni=True, spr=2, ml_nni=20, aa_model=aa)
    if recipe:
        kw.update(RECIPE)
    nj_newick(make, synth.random_descent_codes(200, 64, nc, 0.05, 0.02, seed=42), names[:200], **kw)   # code objects loaded, first launches paid
    t0 = time.perf_counter()
    tree = nj_newick(make, codes, names, **kw)
    whole = time.perf_counter() - t0
    out = dict(case=case, recipe=bool(recipe), call_s=round(whole, 2), tree_crc=zlib.crc32(tree.encode()))
    out.update(last_stage_seconds())
    print(json.dumps(out), flush=True)


def child(case, recipe, limit):
    res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", case, "1" if recipe else "0"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if res.returncode != 0:
        raise SystemExit("FAILED (exit %d): %s, recipe %s:\n%s" % (res.returncode, case, recipe, res.stderr.decode()[-2000:]))
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    if a[:1] == ["--one"]:
        return one(a[1], a[2] == "1")
    arg = lambda k, d: a[a.index(k) + 1] if k in a else d
    out = arg("--out", os.path.join(ROOT, "profiles", "thorough_wallclock.txt"))
    limit = int(arg("--limit", 900))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    emit("# tools/thorough_wallclock.py: the whole pipeline without supports on one MI355X; (a) default, (b) -spr 4 -mlacc 2 -slownni")
    emit("# per run, each in its own process after a warm-up tree: the call's seconds and the stages of vft_nj_last_stage_seconds")
    from veryfasttree_amd import synth
    for case in ("nt", "aa"):
        n, L = CASES[case][:2]
        emit("## %s: %d x %d %s" % (case, n, L, " ".join(CASES[case][6])))
        emit("(a) default: %s" % json.dumps(child(case, False, limit)))
        emit("(b) recipe : %s" % json.dumps(child(case, True, limit)))
        if "--no-reference" in a or not os.path.exists(REFBIN):
            emit("reference: its wall clock was not measured")
            continue
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "a.fa")
            synth.codes_to_fasta(alignment(case), fa, synth.ALPHABET_AA if case == "aa" else synth.ALPHABET_NT)
            cmd = [REFBIN] + CASES[case][6] + ["-spr", "4", "-mlacc", "2", "-slownni", "-nosupport", "-threads", "1", "-seed", "1", fa]
            t0 = time.perf_counter()
            res = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=6000)
            emit("reference, where this tool ran (CPU): VeryFastTree %s (whole program, exit %d) %.2f s" % (" ".join(cmd[1:-1]), res.returncode, time.perf_counter() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
