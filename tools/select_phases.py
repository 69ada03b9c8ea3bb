#!/usr/bin/env python3
"""Where the top-k selection's three kernels spend their time on bench.py's step (8 seeds, 1.25 M ids each, k = 2 000): medians of the
phase clocks that a -DVFT_SELECT_PHASES build stores (vft_kernels_nj.h: VFT_SELPH; thread 0 of workgroup (0, seed), and of the seed's
last workgroup in the rank sort; wall_clock64, 100 MHz).  The clocks only exist in a variant build:

    VFT_EXTRA_HIPCC_FLAGS=-DVFT_SELECT_PHASES python -m veryfasttree_amd.build     # prints the variant's library
    VFT_LIB_DIR=build/variants/<hash> python tools/select_phases.py [steps] > profiles/..._phases.txt

The marks cost a store each and a few waits of their own (VFT_SELPH_USE / VFT_SELPH_DRAIN): read the phases against each other, and
take kernel times from a profiler run of the product library."""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veryfasttree_amd import HipProfileOps, synth
from veryfasttree_amd.workload import TopHitsState

ROWS, SEEDS, MARKS = 4, 16, 8
NAMES = [
    ("k_select_hist, workgroup 0", ["prologue: key range known (min / max reduced, LDS zero)", "criteria binned (loop + barrier)",
                                    "epilogue: global histogram atomics drained"]),
    ("k_select_collect, workgroup 0", ["histogram scanned, threshold digit known", "selection state in registers",
                                       "criteria compacted into LDS (loop + barrier)", "nCand atomic returned (+ barrier)",
                                       "candidate stores drained"]),
    ("k_select_rank, workgroup 0", ["nCand / overflow known", "own candidate + tile staged (last tile)", "compare loop + rank shuffles",
                                    "gathers, publish, vmcnt(0), barrier", "rankDone atomic returned (+ barrier)"]),
    ("k_select_rank, the seed's last workgroup", ["k records fetched, host stores issued", "bestJ known (+ barrier)",
                                                  "__threadfence_system + vmcnt(0) + barrier", "header + release store drained"]),
]


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    n, L = 1000000, 200
    codes = synth.random_descent_codes(n, L, 4, 0.02, 0.01, seed=4)
    ops = HipProfileOps(n, L, 4, np.float32)
    if not hasattr(ops.lib, "vft_debug_select_phases"):
        sys.exit("this library has no phase clocks: build with VFT_EXTRA_HIPCC_FLAGS=-DVFT_SELECT_PHASES and set VFT_LIB_DIR")
    st = TopHitsState(ops, codes, n // 4)
    k = 2 * int(0.5 + np.sqrt(n))
    leaf_act, int_act = st.active[st.active < n], st.active[st.active >= n]
    seeds = []
    for s in range(4):   # bench.py's step: 4 leaf seeds and 4 profile seeds
        seeds.append(int(leaf_act[(s * 7919 + 13) % len(leaf_act)]))
        seeds.append(int(int_act[(s * 104729 + 7) % len(int_act)]))
    seeds = np.asarray(seeds, np.int64)
    buf = np.zeros((ROWS, SEEDS, MARKS), np.uint64)
    runs = []
    for it in range(3 + steps):
        ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k, view=True)
        rc = ops.lib.vft_debug_select_phases(ops.ctx, buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.size))
        if rc != 0:
            sys.exit("vft_debug_select_phases: %s" % ops.lib.vft_last_error(ops.ctx).decode())
        if it >= 3:
            runs.append(buf[:, :len(seeds), :].astype(np.int64))
    t = np.stack(runs) / 100.0   # [run][row][seed][mark], us
    print("# top-k selection phase clocks: bench.py's step (%d seeds, %d ids each, k = %d), %d steps after 3 warm-up steps" % (
        len(seeds), st.maxnode, k, steps))
    print("# median over steps and seeds of (mark - previous mark), us; [min .. max]; wall_clock64 ticks of 10 ns")
    for r, (title, names) in enumerate(NAMES):
        print("%s" % title)
        for m, name in enumerate(names, start=1):
            d = (t[:, r, :, m] - t[:, r, :, m - 1]).ravel()
            print("  %-62s %7.2f  [%6.2f .. %6.2f]" % (name, np.median(d), d.min(), d.max()))
        d = (t[:, r, :, len(names)] - t[:, r, :, 0]).ravel()
        print("  %-62s %7.2f  [%6.2f .. %6.2f]" % ("= first mark to last mark", np.median(d), d.min(), d.max()))
    print("between the kernels (workgroup 0's clocks; the other workgroups end later and start earlier)")
    for name, gap in (("hist's last mark -> collect's first", t[:, 1, :, 0] - t[:, 0, :, 3]),
                      ("collect's last mark -> rank's first", t[:, 2, :, 0] - t[:, 1, :, 5]),
                      ("rank: workgroup 0 done -> the last workgroup knows it is last", t[:, 3, :, 0] - t[:, 2, :, 5])):
        d = gap.ravel()
        print("  %-62s %7.2f  [%6.2f .. %6.2f]" % (name, np.median(d), d.min(), d.max()))
    # the whole selection of a step: the earliest first mark of hist to the latest release store, over the seeds
    whole = t[:, 3, :, 4].max(axis=1) - t[:, 0, :, 0].min(axis=1)
    print("the selection of a step, hist's first mark to the last seed's release store: median %.2f us  [%.2f .. %.2f]" % (
        np.median(whole), whole.min(), whole.max()))


if __name__ == "__main__":
    main()
