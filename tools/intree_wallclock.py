#!/usr/bin/env python3
"""Wall-clock of `-intree T -nome -mllen`: ML branch lengths and SH-like supports on a given topology, no NJ phase.

    intree_wallclock.py [--out profiles/intree_wallclock.txt] [--n 10000] [--pos 1000]

At n x pos nucleotides (synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=41)):
  1. the start tree T is this backend's own `-noml -nome -nosupport` tree of the alignment (tools/nj_tree.py in.fasta -nosupport);
  2. `tools/nj_tree.py in.fasta -intree T -mllen` as a whole program, and in one process for vft_nj_last_stage_seconds' split (slot 0 is the
     time to read the tree and build the profiles);
  3. `VeryFastTree -nt -threads 1 -seed 1 -intree T -nome -mllen` when oracle/_ref/VeryFastTree is there; the two outputs must be
     byte-identical (asserted).
No threshold: the figures go to the output file.  Every GPU step runs in its own child process with its own time limit; the first failure
ends the run."""
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


def split(n, pos, nwk):
    """one run in this process: prints the stage split as one JSON line"""
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import nj_newick, last_stage_seconds, last_join_crcs
    codes = synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=41)
    names = ["s%d" % k for k in range(n)]
    with open(nwk) as fh:
        text = fh.read()
    make = lambda m, L: HipProfileOps(m, L, 4, np.float32, max_nodes=3 * m)
    warm = synth.random_descent_codes(200, 64, 4, 0.05, 0.02, seed=42)
    nj_newick(make, warm, names[:200], me_lengths=True, mllen=20, n_bootstrap=1000)   # code objects loaded, first-launch costs paid
    t0 = time.perf_counter()
    nj_newick(make, codes, names, me_lengths=True, mllen=20, n_bootstrap=1000, intree=text)
    whole = time.perf_counter() - t0
    st = last_stage_seconds()
    print(json.dumps({"n": n, "pos": pos, "nj_newick_call_s": round(whole, 3), "read_tree_and_profiles_s": st["nj"],
                      "me_lengths_supports_s": st["me_lengths_supports"], "ml_stage_s": st["ml_stage"],
                      "of_which_sh_supports_s": st["of_which_sh_supports"], "of_which_model_fits_s": st["of_which_model_fits"],
                      "joins": last_join_crcs()[1]}), flush=True)


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
        return split(int(a[1]), int(a[2]), a[3])
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "intree_wallclock.txt")
    n = int(a[a.index("--n") + 1]) if "--n" in a else 10000
    pos = int(a[a.index("--pos") + 1]) if "--pos" in a else 1000
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    from veryfasttree_amd import synth
    emit("# tools/intree_wallclock.py: -intree T -nome -mllen on one MI355X (float, CAT 20, 1000 resamples), %d x %d nucleotides; one run each" % (n, pos))
    with tempfile.TemporaryDirectory() as tmp:
        fa, nwk = os.path.join(tmp, "a.fa"), os.path.join(tmp, "start.nwk")
        synth.codes_to_fasta(synth.random_descent_codes(n, pos, 4, 0.05, 0.02, seed=41), fa, synth.ALPHABET_NT)
        t_start = timed([sys.executable, NJ_TREE, fa, "-nosupport"], nwk, 900)
        emit("start tree T: tools/nj_tree.py -nosupport (NJ, ME lengths; whole program) %.2f s, %d bytes" % (t_start, os.path.getsize(nwk)))
        ours_out, ref_out = os.path.join(tmp, "ours.nwk"), os.path.join(tmp, "ref.nwk")
        ours = timed([sys.executable, NJ_TREE, fa, "-intree", nwk, "-mllen"], ours_out, 900)
        emit("tools/nj_tree.py -intree T -mllen (whole program: interpreter start, FASTA, context, parse, profiles, ME lengths, ML lengths, supports) %.2f s" % ours)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--split", str(n), str(pos), nwk], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=900)
        if res.returncode != 0:
            emit("FAILED (exit %d) in the stage split: %s" % (res.returncode, res.stderr.decode()[-2000:]))
            return 1
        emit("vft_nj_last_stage_seconds of the same run in a warm process: " + res.stdout.decode().strip())
        if os.path.exists(REFBIN):
            ref = timed([REFBIN, "-nt", "-threads", "1", "-seed", "1", "-intree", nwk, "-nome", "-mllen", fa], ref_out, 3000)
            same = open(ref_out, "rb").read() == open(ours_out, "rb").read()
            emit("VeryFastTree -nt -threads 1 -seed 1 -intree T -nome -mllen (whole program) %.2f s; outputs byte-identical: %s" % (ref, same))
            assert same, "the outputs differ"
        else:
            emit("reference binary not present: its wall time was not measured and the outputs were not compared")
    return 0


if __name__ == "__main__":
    sys.exit(main())
