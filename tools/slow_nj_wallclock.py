#!/usr/bin/env python3
"""Wall-clock of the NJ phase under `-slow` (exhaustive search on the device-resident distance matrix, vft_exhaustive_*).

    slow_nj_wallclock.py                    # 1500 x 80, 5000 x 200, 20000 x 200 (synthetic), a fresh process each, and the
                                            # reference's own -slow at 1500 x 80 with 1 and 16 threads when oracle/_ref is there
    slow_nj_wallclock.py --one N L          # one size in this process (what rocprofv3 --kernel-trace --stats wraps)
    slow_nj_wallclock.py --stats CSV N      # a rocprofv3 kernel-stats CSV of `--one N L` -> device time per part of a join,
                                            # and the search kernel's bytes per second against the bytes it reads

Per size: wall time of vft_nj_run (leaf upload, out-profile, matrix fill and all joins; the call returns after the last
wait), the host's view per entry point (VFT_NJ_PROFILE: time inside each call - vft_exhaustive_search is the one that waits,
so its time is the device's backlog of that join plus the search), and the CRC of the join order (vft_nj_last_join_crcs).
The join orders at 5 000 and 20 000 sequences have no reference to compare with - the reference's -slow grows with N^3 L and
is not affordable beyond about 3 000 sequences - so their CRCs are SELF-RECORDED: they pin later changes, not correctness."""
import csv
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1500, 80), (5000, 200), (20000, 200)]
HBM_ACHIEVABLE = 6.3e12   # bytes / s


def alignment(n, L):
    from veryfasttree_amd import synth
    codes = synth.random_descent_codes(n, L, 4, 0.03, 0.01, seed=23 if (n, L) == (1500, 80) else 3)
    _, first = np.unique(codes, axis=0, return_index=True)
    return codes[np.sort(first)]


def search_bytes(n, itemsize=4):
    """(upper triangle the kernel reads, n^2 yardstick) summed over the joins n_active = n .. 4"""
    k = np.arange(4, n + 1, dtype=np.float64)
    return float((k * (k - 1) / 2).sum() * itemsize), float((k * k).sum() * itemsize)


def one(n, L):
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import last_join_crcs, nj_run
    codes = alignment(n, L)
    warm = alignment(300, 40)   # code objects loaded, first-launch costs paid
    nj_run(HipProfileOps(warm.shape[0], 40, 4, np.float32), warm, slow=True)
    ops = HipProfileOps(codes.shape[0], L, 4, np.float32)
    t0 = time.perf_counter()
    joins, _ = nj_run(ops, codes, slow=True)
    wall = time.perf_counter() - t0
    chunk, nj, crcs = last_join_crcs()
    tri, sq = search_bytes(codes.shape[0])
    print(json.dumps({"n": n, "L": L, "unique": int(codes.shape[0]), "joins": int(len(joins)), "nj_wall_s": round(wall, 4),
                      "us_per_join": round(1e6 * wall / max(len(joins), 1), 1), "search_bytes_read": tri, "search_bytes_n2": sq,
                      "n2_over_hbm_s": round(sq / HBM_ACHIEVABLE, 4), "join_crcs_self_recorded": ["%08x" % c for c in crcs]}), flush=True)


GROUPS = [("search", r"k_ex_prepare|k_ex_search|k_ex_finish"), ("fill", r"k_ex_mirror|k_pairs_block_tiled"),
          ("row", r"k_ex_move|k_ex_column|k_pairs_block"), ("out-distances", r"OUTDIST|k_out_dist|k_sweep|k_leaf_hist|k_refresh"),
          ("join (profile, out-profile)", r"k_join|k_average|k_out_profile|k_selfdist|k_commit|k_rebuild")]


def stats(path, n):
    rows = list(csv.DictReader(open(path)))
    tot = {g: 0.0 for g, _ in GROUPS}
    tot["other"] = 0.0
    search_ns = calls = 0
    for r in rows:
        ns = float(r["TotalDurationNs"])
        if "k_ex_search" in r["Name"]:
            search_ns += ns
            calls += int(r["Calls"])
        for g, pat in GROUPS:
            if re.search(pat, r["Name"]):
                tot[g] += ns
                break
        else:
            tot["other"] += ns
    print("# device time by part of a join, N = %d (rocprofv3 --kernel-trace --stats; tracing slows the host, so no wall time here;\n"
          "# the warm-up run of 300 x 40 - 239 joins - is in the totals)" % n)
    for g, ns in tot.items():
        print("%-30s %10.3f ms" % (g, ns / 1e6))
    tri, sq = search_bytes(n)
    if search_ns:
        s = search_ns / 1e9
        print("k_ex_search: %d launches, %.4f s in all; reads %.3e bytes (upper triangle) -> %.2f TB/s; sum n^2 x 4 = %.3e bytes, at %.1f TB/s "
              "%.4f s -> ratio (search time / that) %.2f" % (calls, s, tri, tri / s / 1e12, sq, HBM_ACHIEVABLE / 1e12, sq / HBM_ACHIEVABLE, s / (sq / HBM_ACHIEVABLE)))


def reference_1500():
    ref = os.path.join(ROOT, "oracle", "_ref", "VeryFastTree")
    if not os.path.exists(ref):
        print("reference binary not present: its -slow wall time was not measured")
        return
    from veryfasttree_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "a.fa")
        synth.codes_to_fasta(alignment(1500, 80), fa)
        for th in (1, 16):
            t0 = time.perf_counter()
            subprocess.run([ref, "-nt", "-slow", "-threads", str(th), "-noml", "-nome", "-nosupport", fa], stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, check=True)
            print("reference VeryFastTree -nt -slow -noml -nome -nosupport -threads %d, 1500 x 80: %.1f s (whole program)" % (th, time.perf_counter() - t0), flush=True)


def main():
    a = sys.argv[1:]
    if a[:1] == ["--one"]:
        return one(int(a[1]), int(a[2]))
    if a[:1] == ["--stats"]:
        return stats(a[1], int(a[2]))
    env = dict(os.environ, VFT_NJ_PROFILE="1")
    for n, L in SIZES:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), str(L)], env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=900)
        print(res.stdout.decode().strip(), flush=True)
        if res.returncode != 0:
            print("FAILED (exit %d): %s" % (res.returncode, res.stderr.decode()[-2000:]))
            return 1
        # two reports with the same entry points: the warm-up's, then the timed run's
        rep = [l for l in res.stderr.decode().splitlines() if re.search(r"\d+ calls\s+[\d.]+ s", l)]
        print("\n".join(rep[len(rep) // 2:]), flush=True)
    if "--no-reference" not in a:
        reference_1500()
    return 0


if __name__ == "__main__":
    sys.exit(main())
