#!/usr/bin/env python3
"""What `-rawdist` for a tree and `-trans` cost when they are off, and what `-rawdist` costs when it is on: wall-clock of
tools/nj_tree.py's pipeline (`-full`, i.e. `VeryFastTree -nt`: NJ, ME NNIs and SPRs, ML NNIs with 20 rate categories, 1000 SH-like
resamples) on one seeded alignment of 3 000 x 300 nucleotides.

    python tools/distopt_wallclock.py --parent-libs DIR [--runs 5] [--out profiles/distopt_wallclock.txt]

DIR holds libvft_hip.so and libvft_host.so built from the parent commit (a checkout of it, `python -m veryfasttree_amd.build`, its
veryfasttree_amd/lib).  Five alternating rounds of (a) this tree with both options off, (b) the parent's libraries, (c) this tree with
-rawdist; every run is a process of its own (one process loads one pair of libraries) that times nj_newick, context creation included.
(a) against (b) is judged with the spread of (b)'s own runs as the margin: with the options off the walk server's commands carry one
more zero bit, the supports one more compare, and the host one more branch per corrected distance.  (c) is another computation (other
NNIs and SPR moves, another starting point of the ML stage): reported, not bounded."""
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(npy, rawdist):
    """a single timed run in this process: prints the seconds and the tree's CRC-32"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_newick
    from veryfasttree_amd.refflags import from_reference_flags
    codes = np.load(npy)
    run = from_reference_flags("-nt")
    names = ["s%d" % k for k in range(len(codes))]
    t0 = time.perf_counter()
    more = dict(rawdist=True) if rawdist else {}   # (off: vft_set_raw_distances is never called - the parent's library has none)
    tree = nj_newick(lambda n, L: HipProfileOps(n, L, 4, run.dtype, max_nodes=3 * n), codes, names, me_lengths=True, n_bootstrap=run.n_bootstrap,
                     **dict(run.kwargs, **more))
    print("%.4f %08x" % (time.perf_counter() - t0, zlib.crc32(tree.encode())))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--one":
        return one(args[1], len(args) > 2 and args[2] == "rawdist")
    opt = dict(zip(args[::2], args[1::2]))
    parent = opt.get("--parent-libs")
    if not parent or not os.path.exists(os.path.join(parent, "libvft_host.so")):
        sys.exit(__doc__)
    runs = int(opt.get("--runs", 5))
    out = opt.get("--out", os.path.join(ROOT, "profiles", "distopt_wallclock.txt"))
    from veryfasttree_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        npy = os.path.join(tmp, "aln.npy")
        np.save(npy, synth.random_descent_codes(3000, 300, 4, 0.05, 0.02, seed=41))
        variants = [("a: this tree, options off", {}, []), ("b: the parent's libraries", {"VFT_LIB_DIR": os.path.abspath(parent)}, []),
                    ("c: this tree, -rawdist", {}, ["rawdist"])]
        times = {label: [] for label, _, _ in variants}
        trees = {label: set() for label, _, _ in variants}
        for _ in range(runs):
            for label, env, more in variants:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", npy] + more, env=dict(os.environ, **env), check=True,
                                     stdout=subprocess.PIPE, timeout=300)
                seconds, crc = res.stdout.decode().split()
                times[label].append(float(seconds))
                trees[label].add(crc)
    lines = ["-rawdist / -trans: wall-clock of nj_newick (tools/nj_tree.py -full) on 3 000 x 300 nucleotides, %d alternating runs each, seconds" % runs]
    for label, _, _ in variants:
        t = times[label]
        lines.append("%-28s median %.3f  min %.3f  max %.3f  runs %s" % (label, float(np.median(t)), min(t), max(t), " ".join("%.3f" % x for x in t)))
    (la, _, _), (lb, _, _), (lc, _, _) = variants
    a, b, c = times[la], times[lb], times[lc]
    spread = max(b) - min(b)
    diff = float(np.median(a) - np.median(b))
    lines.append("a - b (medians) %+.3f s; the spread of b's own runs is %.3f s: %s" % (diff, spread, "within it" if diff <= spread else "BEYOND IT"))
    lines.append("c - a (medians) %+.3f s with -rawdist on (another tree: reported, not bounded)" % float(np.median(c) - np.median(a)))
    lines.append("a and b returned the same tree in every run, byte for byte (CRC-32 %s): %s" % (" ".join(sorted(trees[la] | trees[lb])), len(trees[la] | trees[lb]) == 1))
    lines.append("c returned one tree in every run (CRC-32 %s), another than a's: %s" % (" ".join(sorted(trees[lc])), len(trees[lc]) == 1 and not (trees[lc] & trees[la])))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
