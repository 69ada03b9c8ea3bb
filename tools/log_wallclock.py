#!/usr/bin/env python3
"""What `-log` costs, and what it costs when it is off: wall-clock of tools/nj_tree.py's pipeline (`-full`, i.e. `VeryFastTree -nt`:
NJ, ME NNIs and SPRs, ML NNIs with 20 rate categories, 1000 SH-like resamples) on one seeded alignment of 3 000 x 300 nucleotides.

    python tools/log_wallclock.py --parent-libs DIR [--runs 5] [--out profiles/log_wallclock.txt]

DIR holds libvft_hip.so and libvft_host.so built from the parent commit (a checkout of it, `python -m veryfasttree_amd.build`, its
veryfasttree_amd/lib).  Five alternating rounds of (a) this tree without a log, (b) the parent's libraries, (c) this tree with a log;
every run is a process of its own (one process loads one pair of libraries) that times nj_newick, context creation included.
(a) against (b) is judged with the spread of (b)'s own runs as the margin - with no log nothing may be formatted, downloaded or counted
that the parent does not; (c) is reported, not bounded."""
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(npy, log):
    """a single timed run in this process: prints the seconds"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_newick
    from veryfasttree_amd.refflags import from_reference_flags
    codes = np.load(npy)
    run = from_reference_flags("-nt")
    names = ["s%d" % k for k in range(len(codes))]
    t0 = time.perf_counter()
    more = dict(log=log) if log else {}   # (without a log vft_nj_set_log is never called: the parent's library has none)
    tree = nj_newick(lambda n, L: HipProfileOps(n, L, 4, run.dtype, max_nodes=3 * n), codes, names, me_lengths=True, n_bootstrap=run.n_bootstrap,
                     **dict(run.kwargs, **more))
    print("%.4f %08x" % (time.perf_counter() - t0, zlib.crc32(tree.encode())))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--one":
        return one(args[1], args[2] if len(args) > 2 else None)
    opt = dict(zip(args[::2], args[1::2]))
    parent = opt.get("--parent-libs")
    if not parent or not os.path.exists(os.path.join(parent, "libvft_host.so")):
        sys.exit(__doc__)
    runs = int(opt.get("--runs", 5))
    out = opt.get("--out", os.path.join(ROOT, "profiles", "log_wallclock.txt"))
    from veryfasttree_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        npy = os.path.join(tmp, "aln.npy")
        np.save(npy, synth.random_descent_codes(3000, 300, 4, 0.05, 0.02, seed=41))
        log = os.path.join(tmp, "run.log")
        variants = [("a: this tree, no log", {}, []), ("b: the parent's libraries", {"VFT_LIB_DIR": os.path.abspath(parent)}, []), ("c: this tree, -log", {}, [log])]
        times = {label: [] for label, _, _ in variants}
        sizes = set()
        for _ in range(runs):
            for label, env, more in variants:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", npy] + more, env=dict(os.environ, **env), check=True,
                                     stdout=subprocess.PIPE, timeout=300)
                seconds, size = res.stdout.decode().split()
                times[label].append(float(seconds))
                sizes.add(size)
        log_bytes, log_lines = os.path.getsize(log), sum(1 for _ in open(log))
    lines = ["-log: wall-clock of nj_newick (tools/nj_tree.py -full) on 3 000 x 300 nucleotides, %d alternating runs each, seconds" % runs]
    for label, _, _ in variants:
        t = times[label]
        lines.append("%-28s median %.3f  min %.3f  max %.3f  runs %s" % (label, float(np.median(t)), min(t), max(t), " ".join("%.3f" % x for x in t)))
    a, b, c = (times[label] for label, _, _ in variants)
    spread = max(b) - min(b)
    diff = float(np.median(a) - np.median(b))
    lines.append("a - b (medians) %+.3f s; the spread of b's own runs is %.3f s: %s" % (diff, spread, "within it" if diff <= spread else "BEYOND IT"))
    lines.append("c - a (medians) %+.3f s for a log of %d lines, %d bytes (reported, not bounded)" % (float(np.median(c) - np.median(a)), log_lines, log_bytes))
    lines.append("every run returned the same tree, byte for byte (CRC-32 %s): %s" % (" ".join(sorted(sizes)), len(sizes) == 1))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
