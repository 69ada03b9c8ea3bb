#!/usr/bin/env python3
"""Wall-clock of the default pipeline (`-nt -noml -nome`: NJ, ME lengths, local-bootstrap supports) on an alignment beyond the 1 706
columns of k_split_support, where the supports go through k_split_support_long.

    supports_wallclock.py [--out profiles/supports_long_wallclock.txt] [--n 2000] [--pos 4000]

At n x pos nucleotides (synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=43)):
  1. `tools/nj_tree.py in.fasta` as a whole program;
  2. the same call in one warm process for vft_nj_last_stage_seconds' split ("ME branch lengths + local supports" is one slot);
  3. `VeryFastTree -nt -noml -nome -threads 1` when oracle/_ref/VeryFastTree is there; the two outputs must be byte-identical (asserted).
No threshold: the figures go to the output file.  Every GPU step runs in its own child process with its own time limit, one after the
other, nothing else on the device; the first failure ends the run."""
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
NJ_TREE = os.path.join(ROOT, "tools", "nj_tree.py")
SEED = 43


def split(n, pos):
    """one run in this process: prints the stage split as one JSON line"""
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import nj_newick, last_stage_seconds
    codes = synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=SEED)
    names = ["s%d" % k for k in range(n)]
    make = lambda m, L: HipProfileOps(m, L, 4, np.float32, max_nodes=3 * m)
    warm = synth.random_descent_codes(64, pos, 4, 0.05, 0.02, seed=SEED + 1)
    nj_newick(make, warm, names[:64], me_lengths=True, n_bootstrap=1000)   # code objects loaded, first-launch costs paid
    t0 = time.perf_counter()
    nj_newick(make, codes, names, me_lengths=True, n_bootstrap=1000)
    whole = time.perf_counter() - t0
    st = last_stage_seconds()
    print(json.dumps({"n": n, "pos": pos, "nj_newick_call_s": round(whole, 3), "nj_s": st["nj"],
                      "me_lengths_supports_s": st["me_lengths_supports"]}), flush=True)


def timed(cmd, out_path, limit):
    with open(out_path, "wb") as fh:
        t0 = time.perf_counter()
        res = subprocess.run(cmd, stdout=fh, stderr=subprocess.PIPE, timeout=limit)
        wall = time.perf_counter() - t0
    if res.returncode != 0:
        raise SystemExit("FAILED (exit %d): %s\n%s" % (res.returncode, " ".join(cmd), res.stderr.decode()[-2000:]))
    return wall


def main():
    a = sys.argv[1:]
    if a[:1] == ["--split"]:
        return split(int(a[1]), int(a[2]))
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "supports_long_wallclock.txt")
    n = int(a[a.index("--n") + 1]) if "--n" in a else 2000
    pos = int(a[a.index("--pos") + 1]) if "--pos" in a else 4000
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    from veryfasttree_amd import synth
    emit("# tools/supports_wallclock.py: -nt -noml -nome on one MI355X (float, 1000 resamples), %d x %d nucleotides; one run each" % (n, pos))
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "a.fa")
        synth.codes_to_fasta(synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=SEED), fa, synth.ALPHABET_NT)
        ours_out, ref_out = os.path.join(tmp, "ours.nwk"), os.path.join(tmp, "ref.nwk")
        ours = timed([sys.executable, NJ_TREE, fa], ours_out, 600)
        emit("tools/nj_tree.py (whole program: interpreter start, FASTA, context, NJ, ME lengths, local supports) %.2f s" % ours)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--split", str(n), str(pos)], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=600)
        if res.returncode != 0:
            emit("FAILED (exit %d) in the stage split: %s" % (res.returncode, res.stderr.decode()[-2000:]))
            return 1
        emit("vft_nj_last_stage_seconds of the same run in a warm process: " + res.stdout.decode().strip())
        if os.path.exists(REFBIN):
            ref = timed([REFBIN, "-nt", "-noml", "-nome", "-threads", "1", fa], ref_out, 3000)
            same = open(ref_out, "rb").read() == open(ours_out, "rb").read()
            emit("VeryFastTree -nt -noml -nome -threads 1 (whole program) %.2f s; outputs byte-identical: %s" % (ref, same))
            assert same, "the outputs differ"
        else:
            emit("reference binary not present: its wall time was not measured and the outputs were not compared")
    return 0


if __name__ == "__main__":
    sys.exit(main())
