#!/usr/bin/env python3
"""Where the kinds of workgroup of k_sweep_nt_mixed_multi lie in the kernel's time on bench.py's step (1 M x 200 nt, 4 leaf + 4 profile
seeds): thread 0 of EVERY workgroup stores its kind, whether any of its targets was active, and wall_clock64 (100 MHz) at entry and at
exit (vft_kernels_nj.h: VFT_SWCLK).  The clocks only exist in a variant build:

    VFT_EXTRA_HIPCC_FLAGS=-DVFT_SWEEP_WG_CLOCKS python -m veryfasttree_amd.build     # prints the variant's library
    VFT_LIB_DIR=build/variants/<hash> python tools/sweep_wg_clocks.py [steps] > profiles/..._wg_clocks.txt

("-DVFT_SWEEP_WG_CLOCKS -DVFT_NO_SHARED_LEAF_WALK" gives the same picture of the kernel with its three kinds of workgroup.)
The marks cost two clock reads, one barrier and three stores per workgroup: read the kinds against each other, and take kernel times
from a profiler run of the product library."""
import ctypes as C
import os
import sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from veryfasttree_amd import HipProfileOps, synth
from veryfasttree_amd.workload import TopHitsState

MAX_WG, WORDS = 8192, 3
KINDS = {1: "1 internal targets, all seeds", 2: "2 leaves, leaf seeds (a leaf per lane)", 3: "3 leaf span, table walk (profile seeds)",
         4: "3 leaf span, shared walk (all seeds)"}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    n, L = 1000000, 200
    codes = synth.random_descent_codes(n, L, 4, 0.02, 0.01, seed=4)
    ops = HipProfileOps(n, L, 4, np.float32)
    if not hasattr(ops.lib, "vft_debug_sweep_wg_clocks"):
        sys.exit("this library has no workgroup clocks: build with VFT_EXTRA_HIPCC_FLAGS=-DVFT_SWEEP_WG_CLOCKS and set VFT_LIB_DIR")
    st = TopHitsState(ops, codes, n // 4)
    k = 2 * int(0.5 + np.sqrt(n))
    leaf_act, int_act = st.active[st.active < n], st.active[st.active >= n]
    seeds = []
    for s in range(4):   # bench.py's step: 4 leaf seeds and 4 profile seeds
        seeds.append(int(leaf_act[(s * 7919 + 13) % len(leaf_act)]))
        seeds.append(int(int_act[(s * 104729 + 7) % len(int_act)]))
    seeds = np.asarray(seeds, np.int64)
    buf = np.zeros((MAX_WG, WORDS), np.uint64)
    runs = []
    for it in range(3 + steps):
        ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k, view=True)
        rc = ops.lib.vft_debug_sweep_wg_clocks(ops.ctx, buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.size))
        if rc != 0:
            sys.exit("vft_debug_sweep_wg_clocks: %s" % ops.lib.vft_last_error(ops.ctx).decode())
        if it >= 3:
            runs.append(buf.astype(np.int64))
    print("# k_sweep_nt_mixed_multi, workgroup clocks: bench.py's step (%d seeds, %d ids), %d steps after 3 warm-up steps" % (
        len(seeds), st.maxnode, steps))
    print("# us relative to the kernel's first mark; median over the steps [min .. max]; wall_clock64 ticks of 10 ns")
    rows = {}
    spans = []
    for r in runs:
        tag = r[:, 0]
        ok = tag != 0
        kind, worked = tag[ok] & 15, (tag[ok] >> 4) & 1
        t0 = r[ok, 1].min()
        start, end = (r[ok, 1] - t0) / 100.0, (r[ok, 2] - t0) / 100.0
        spans.append(end.max())
        for kd in np.unique(kind):
            for w in (1, 0):
                m = (kind == kd) & (worked == w)
                if not m.any():
                    continue
                d = end[m] - start[m]
                rows.setdefault((int(kd), w), []).append((m.sum(), start[m].min(), np.median(start[m]), start[m].max(), end[m].max(),
                                                          np.median(d), d.max(), d.sum()))
    print("%-44s %6s %9s %9s %9s %9s %9s %9s %11s" % ("kind", "count", "1st start", "med start", "last strt", "last end", "med dur",
                                                      "max dur", "sum dur"))
    for (kd, w), v in sorted(rows.items()):
        a = np.median(np.asarray(v, float), axis=0)
        print("%-44s %6d %9.1f %9.1f %9.1f %9.1f %9.2f %9.2f %11.0f" % (
            KINDS.get(kd, str(kd)) + (", worked" if w else ", sentinels only"), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]))
    spans = np.asarray(spans)
    print("the kernel's span, first mark to last: median %.1f us  [%.1f .. %.1f]" % (np.median(spans), spans.min(), spans.max()))
    # how far the kinds overlap: the time at which the last working internal workgroup ends, and the share of the leaf kinds' summed
    # durations that lies behind it
    r = runs[len(runs) // 2]
    ok = r[:, 0] != 0
    kind, worked = r[ok, 0] & 15, (r[ok, 0] >> 4) & 1
    t0 = r[ok, 1].min()
    start, end = (r[ok, 1] - t0) / 100.0, (r[ok, 2] - t0) / 100.0
    m1 = (kind == 1) & (worked == 1)
    if m1.any():
        e1 = end[m1].max()
        print("one step: the last working internal workgroup ends at %.1f us; 95 %% of them have ended by %.1f us" % (
            e1, np.percentile(end[m1], 95)))
        for kd in (2, 3, 4):
            m = (kind == kd) & (worked == 1)
            if m.any():
                behind = np.clip(end[m] - np.maximum(start[m], e1), 0, None).sum()
                print("  kind %d: %.0f of %.0f workgroup-us lie behind that point; its last workgroup ends at %.1f us" % (
                    kd if kd < 4 else 3, behind, (end[m] - start[m]).sum(), end[m].max()))


if __name__ == "__main__":
    main()
