#!/usr/bin/env python3
"""What `-pseudo` costs in the SPR stage, and that a run WITHOUT it pays nothing for the walk server's new weight answer.

    pseudo_wallclock.py --parent-lib DIR [--out profiles/pseudo_wallclock.txt] [--n 10000] [--pos 200] [--repeats 5]

Input: a fragment alignment of a size a user would run - tools/gen_pseudo_fixtures.py's generator, n x pos nucleotides (seed 14), every
row one window of 30 % of the columns.  Timed: the `-noml` pipeline (NJ, ME NNIs + 2 SPR rounds, ME lengths; no supports),
  (a) with the libraries of the PARENT commit (DIR holds its libvft_hip.so and libvft_host.so, loaded through VFT_LIB_DIR),
  (b) with this commit's, pseudo = 0,
  (c) with this commit's, pseudo = 1.
(a) and (b) alternate, `repeats` times each, every run in a child process of its own (one library pair per process) after a warm-up
tree in that process; then (c) once.  Per run: the SPR stage's seconds and chain steps (vft_nj_last_stage_seconds) and the time per
step.  The condition: (b)'s mean time per step lies within the spread (min .. max) of (a)'s repeats - or below it.  (c) is reported with
its cause (no dual commands are sent while pseudo > 0).  The reference's wall clock for the same command is timed where the tool runs
when oracle/_ref/VeryFastTree is there.  Every GPU step runs under a time limit of its own; the first failure ends the run."""
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


def alignment(n, pos):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_pseudo_fixtures import fragments
    return fragments(n, pos, 4, 14, 0.30)()


def one(n, pos, pseudo):
    """one run in this process (the libraries are whatever VFT_LIB_DIR says): prints one JSON line"""
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import nj_newick, last_stage_seconds
    codes = alignment(n, pos)
    names = ["s%d" % k for k in range(n)]
    make = lambda m, L: HipProfileOps(m, L, 4, np.float32, max_nodes=3 * m)
    kw = dict(me_lengths=True, me_nni=True, spr=2)
    if pseudo > 0:
        kw["pseudo"] = pseudo
    nj_newick(make, synth.random_descent_codes(300, 64, 4, 0.05, 0.02, seed=42), names[:300], **kw)   # code objects loaded, first launches paid
    t0 = time.perf_counter()
    tree = nj_newick(make, codes, names, **kw)
    whole = time.perf_counter() - t0
    st = last_stage_seconds()
    import zlib
    print(json.dumps({"pseudo": pseudo, "call_s": round(whole, 3), "spr_s": st["of_which_spr"], "spr_steps": st["spr_steps"],
                      "spr_moves": st["spr_moves"], "dual_commands": st["spr_dual_commands"], "dual_taken": st["spr_dual_continuations"],
                      "us_per_step": round(1e6 * st["of_which_spr"] / max(st["spr_steps"], 1), 3), "tree_crc": zlib.crc32(tree.encode())}), flush=True)


def child(n, pos, pseudo, lib_dir, limit):
    env = dict(os.environ)
    env.pop("VFT_LIB_DIR", None)
    if lib_dir:
        env["VFT_LIB_DIR"] = lib_dir
    res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", str(n), str(pos), str(pseudo)],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    if res.returncode != 0:
        raise SystemExit("FAILED (exit %d) with pseudo %s, libraries %s:\n%s" % (res.returncode, pseudo, lib_dir or "this commit's", res.stderr.decode()[-2000:]))
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    a = sys.argv[1:]
    if a[:1] == ["--one"]:
        return one(int(a[1]), int(a[2]), float(a[3]))
    arg = lambda k, d: a[a.index(k) + 1] if k in a else d
    out = arg("--out", os.path.join(ROOT, "profiles", "pseudo_wallclock.txt"))
    n, pos, repeats, limit = int(arg("--n", 10000)), int(arg("--pos", 200)), int(arg("--repeats", 5)), int(arg("--limit", 150))
    parent = arg("--parent-lib", None)
    if not parent or not os.path.exists(os.path.join(parent, "libvft_host.so")):
        raise SystemExit("--parent-lib DIR: the parent commit's libvft_hip.so and libvft_host.so (build the parent in a worktree)")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    emit("# tools/pseudo_wallclock.py: the -noml pipeline (NJ, ME NNIs, 2 SPR rounds, ME lengths; float) on one MI355X, a fragment alignment of "
         "%d x %d nucleotides (30 %% of the columns per row)" % (n, pos))
    emit("# per run, each in its own process after a warm-up tree: SPR stage seconds, chain steps, microseconds per step (vft_nj_last_stage_seconds)")
    A, B = [], []
    for r in range(repeats):
        A.append(child(n, pos, 0.0, parent, limit))
        emit("(a) parent commit          run %d: %s" % (r + 1, json.dumps(A[-1])))
        B.append(child(n, pos, 0.0, None, limit))
        emit("(b) this commit, pseudo=0  run %d: %s" % (r + 1, json.dumps(B[-1])))
    ua, ub = [x["us_per_step"] for x in A], [x["us_per_step"] for x in B]
    same_tree = len({x["tree_crc"] for x in A + B}) == 1 and len({x["spr_steps"] for x in A + B}) == 1
    emit("(a) us per step: min %.3f mean %.3f max %.3f   (b) us per step: min %.3f mean %.3f max %.3f   same tree and step count in all runs: %s"
         % (min(ua), sum(ua) / len(ua), max(ua), min(ub), sum(ub) / len(ub), max(ub), same_tree))
    ok = sum(ub) / len(ub) <= max(ua)
    emit("condition - (b)'s mean within (or below) the spread of (a)'s repeats: %s" % ("met" if ok else "NOT met"))
    c = child(n, pos, 1.0, None, limit)
    emit("(c) this commit, pseudo=1        : %s" % json.dumps(c))
    emit("(c) sends no dual commands (dual_commands 0): every chain step waits for the host's verdict, as with VFT_NJ_DEBUG_NO_WALK_DUAL, and "
         "its answer carries six more granules; its tree and step count are another run's (pseudocount distances), so its time per step, not its stage time, compares with (b)")
    if os.path.exists(REFBIN):
        from veryfasttree_amd import synth
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "a.fa")
            synth.codes_to_fasta(alignment(n, pos), fa, synth.ALPHABET_NT)
            for flags in ([], ["-pseudo"]):
                t0 = time.perf_counter()
                res = subprocess.run([REFBIN, "-nt", "-noml", "-nosupport", "-threads", "1", "-seed", "1"] + flags + [fa], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=3000)
                emit("reference, where this tool ran (CPU): VeryFastTree -nt -noml -nosupport -threads 1 %s (whole program, exit %d) %.2f s"
                     % (" ".join(flags), res.returncode, time.perf_counter() - t0))
    else:
        emit("reference binary not present: its wall clock was not measured")
    return 0 if ok and same_tree else 1


if __name__ == "__main__":
    sys.exit(main())
