#!/usr/bin/env python3
"""Wall clock of the ML stage with and without `-approxml`, against the parent commit's libraries, on one MI355X:

    python tools/approxml_wallclock.py --parent-libs DIR [--runs 5] [--out profiles/approxml_wallclock.txt]

DIR holds libvft_hip.so and libvft_host.so built from the parent commit (veryfasttree_amd/build.py in a checkout of it).  Two
alignments - 3 000 x 300 `-lg -double-precision` and 3 000 x 300 JTT float - and three variants: the parent's libraries, this tree
with the switch off, this tree with it on.  Every run is a process of its own (a library is chosen when it is loaded); the variants
alternate, `--runs` times each, so that drift of the machine lands on all three alike.  Printed per variant: the median and the spread
(least - most) of the ML stage's seconds (backend.last_stage_seconds: ml_stage) and of the whole call.

What the figures have to show: the switch off costs no more than the parent beyond the spread of the parent's own runs.  With the
switch on the figure is reported, whatever it is."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("lg_double_3000x300", "-lg -double-precision", 41), ("jtt_float_3000x300", "", 42)]
N, L = 3000, 300


def child(flags, seed):
    sys.path.insert(0, ROOT)
    import numpy as np  # noqa: F401
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import last_stage_seconds, nj_newick
    from veryfasttree_amd.refflags import from_reference_flags
    run = from_reference_flags(flags)
    codes = synth.random_descent_codes(N, L, 20, 0.08, 0.02, seed)
    names = ["s%d" % k for k in range(len(codes))]
    t0 = time.perf_counter()
    tree, loglk = nj_newick(lambda n, Lp: HipProfileOps(n, Lp, run.n_codes, run.dtype, max_nodes=3 * n), codes, names, me_lengths=True,
                            n_bootstrap=run.n_bootstrap, return_loglk=True, **run.kwargs)
    wall = time.perf_counter() - t0
    st = last_stage_seconds()
    print(json.dumps(dict(wall=wall, ml_stage=st["ml_stage"], loglk=float(loglk[-1]), tree_bytes=len(tree))))


def one(flags, seed, lib_dir):
    env = dict(os.environ)
    if lib_dir:
        env["VFT_LIB_DIR"] = lib_dir
    else:
        env.pop("VFT_LIB_DIR", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", flags, str(seed)], env=env, stdout=subprocess.PIPE, timeout=600, check=True)
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        return child(args[1], int(args[2]))
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d
    parent = opt("--parent-libs", None)
    if not parent or not os.path.exists(os.path.join(parent, "libvft_hip.so")):
        sys.exit(__doc__)
    runs, out = int(opt("--runs", "5")), opt("--out", None)
    lines = ["# tools/approxml_wallclock.py: %d x %d proteins, %d alternating runs per variant, seconds: median (least - most)" % (N, L, runs)]
    for name, flags, seed in CASES:
        variants = [("parent", flags, os.path.abspath(parent)), ("change, exact", flags, None), ("change, -approxml", (flags + " -approxml").strip(), None)]
        got = {v[0]: [] for v in variants}
        for _ in range(runs):
            for label, fl, lib in variants:
                got[label].append(one(fl, seed, lib))
                print(name, label, got[label][-1], flush=True)
        lines.append("%s  (VeryFastTree %s)" % (name, flags or "<no flags>"))
        for label, _, _ in variants:
            ml, wall = [g["ml_stage"] for g in got[label]], [g["wall"] for g in got[label]]
            lines.append("  %-18s ml_stage %7.2f (%7.2f - %7.2f)   whole call %7.2f (%7.2f - %7.2f)   final logLk %.3f" % (
                label, statistics.median(ml), min(ml), max(ml), statistics.median(wall), min(wall), max(wall), got[label][-1]["loglk"]))
        assert got["parent"][-1]["loglk"] == got["change, exact"][-1]["loglk"], "the exact path computes something else than the parent"
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
