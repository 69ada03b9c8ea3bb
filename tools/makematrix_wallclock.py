#!/usr/bin/env python3
"""Wall-clock of `-makematrix` (all-pairs distances: vft_seq_matrix_rows + the slab driver vft_nj_make_matrix).

    makematrix_wallclock.py [--out profiles/makematrix_wallclock.txt] [--no-reference] [--no-large]

1. Against the reference, when oracle/_ref/VeryFastTree is there: the same FASTA at 3 000 x 500 nucleotides and 3 000 x 300 proteins,
   float, output to a file - `VeryFastTree [-nt] -makematrix -threads 1` and `tools/nj_tree.py -makematrix [-aa]`, each as a whole
   program, once after a warm-up run; the two outputs must be byte-identical (asserted).
2. This project alone at 20 000 x 1 000 nucleotides and 20 000 x 300 proteins, output to /dev/null: leaf upload; kernel time summed
   from stream events (slab by slab, no copy); the device-to-host copies of the same slabs into page-locked memory; and the driver's
   own split of a whole run (waiting for the device, formatting, write).  For the kernels: achieved column comparisons per second.

Every GPU step runs in its own child process with its own time limit; the first failure ends the run."""
import ctypes as C
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

COMPARE = [("nt", 3000, 500), ("aa", 3000, 300)]
LARGE = [("nt", 20000, 1000), ("aa", 20000, 300)]


def alignment(kind, n, L):
    from veryfasttree_amd import synth
    return synth.random_descent_codes(n, L, 4 if kind == "nt" else 20, 0.05 if kind == "nt" else 0.10, 0.02, seed=31 if kind == "nt" else 32)


def split(kind, n, L):
    """one size in this process: prints one JSON line"""
    from veryfasttree_amd import HipProfileOps, backend
    from veryfasttree_amd.backend import I32, I64, P
    codes = alignment(kind, n, L)
    nc = 4 if kind == "nt" else 20
    names = ["s%d" % k for k in range(n)]
    devnull = os.open(os.devnull, os.O_WRONLY)
    warm = alignment(kind, 200, 64)
    backend.make_matrix(warm, names[:200], nc, np.float32, False, devnull)   # code objects loaded, first-launch costs paid
    ops = HipProfileOps(n, L, nc, np.float32, max_nodes=n)
    t0 = time.perf_counter()
    ops.upload_leaves(codes)
    upload = time.perf_counter() - t0
    if nc == 20:
        t = backend.distance_tables(None, np.float32)
        ops.set_distance_matrix(t["distances"], t["codefreq"], t["eigenval"], t["eigentot"])
    ld = (n + 63) & ~63
    rows = max(1, min(n, (256 << 20) // (4 * ld * 4)))   # the driver's default slab (host/SeqMatrix.h)
    d_out, h_out = P(), P()
    ops._chk(ops.lib.vft_device_malloc(ops.ctx, I64(rows * ld * 4), C.byref(d_out)))
    ops._chk(ops.lib.vft_host_malloc(ops.ctx, I64(rows * ld * 4), C.byref(h_out)))
    kernel_ms = copy_s = 0.0
    slabs = 0
    for r0 in range(0, n, rows):
        r1 = min(r0 + rows, n)
        ops.timer_start()
        ops._chk(ops.lib.vft_seq_matrix_rows(ops.ctx, I64(r0), I64(r1), I32(1), d_out, I64(ld), None))
        kernel_ms += ops.timer_stop_ms()
        t0 = time.perf_counter()
        ops._chk(ops.lib.vft_download_async(ops.ctx, h_out, d_out, I64((r1 - r0) * ld * 4), I32(0)))
        ops._chk(ops.lib.vft_download_wait(ops.ctx, I32(0)))
        copy_s += time.perf_counter() - t0
        slabs += 1
    ops._chk(ops.lib.vft_host_free(ops.ctx, h_out))
    ops._chk(ops.lib.vft_device_free(ops.ctx, d_out))
    ops.close()
    t0 = time.perf_counter()
    drv = backend.make_matrix(codes, names, nc, np.float32, False, devnull, return_times=True)
    whole = time.perf_counter() - t0
    os.close(devnull)
    comparisons = float(n) * n * L
    print(json.dumps({"kind": kind, "n": n, "L": L, "slab_rows": rows, "slabs": slabs, "upload_s": round(upload, 4),
                      "kernel_s_from_events": round(kernel_ms / 1e3, 4), "d2h_copy_s": round(copy_s, 4),
                      "column_comparisons": comparisons, "column_comparisons_per_s": round(comparisons / (kernel_ms / 1e3), 0),
                      "driver_wait_for_device_s": round(drv["device_wait"], 4), "driver_format_s": round(drv["format"], 4),
                      "driver_write_s": round(drv["write"], 4), "driver_total_s": round(drv["total"], 4),
                      "make_matrix_call_s": round(whole, 4), "bytes_written": drv["bytes"]}), flush=True)


def timed(cmd, out_path, limit):
    with open(out_path, "wb") as fh:
        t0 = time.perf_counter()
        res = subprocess.run(cmd, stdout=fh, stderr=subprocess.PIPE, timeout=limit)
        wall = time.perf_counter() - t0
    if res.returncode != 0:
        raise SystemExit("FAILED (exit %d): %s\n%s" % (res.returncode, " ".join(cmd), res.stderr.decode()[-2000:]))
    return wall


def compare(kind, n, L, emit):
    from veryfasttree_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "a.fa")
        synth.codes_to_fasta(alignment(kind, n, L), fa, synth.ALPHABET_NT if kind == "nt" else synth.ALPHABET_AA)
        ref_cmd = [REFBIN] + (["-nt"] if kind == "nt" else []) + ["-makematrix", "-threads", "1", fa]
        our_cmd = [sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), "-makematrix"] + (["-aa"] if kind == "aa" else []) + [fa]
        ref_out, our_out = os.path.join(tmp, "ref.txt"), os.path.join(tmp, "our.txt")
        timed(our_cmd, our_out, 300)                 # warm-up
        ours = timed(our_cmd, our_out, 300)
        timed(ref_cmd, ref_out, 600)                 # warm-up
        ref = timed(ref_cmd, ref_out, 600)
        same = open(ref_out, "rb").read() == open(our_out, "rb").read()
        emit("%s %d x %d, float, output to a file (%d bytes): reference (-threads 1, whole program) %.2f s; tools/nj_tree.py -makematrix "
             "(whole program: interpreter start, context, upload, matrix, text) %.2f s; outputs byte-identical: %s"
             % (kind, n, L, os.path.getsize(ref_out), ref, ours, same))
        assert same, "the outputs differ"


def main():
    a = sys.argv[1:]
    if a[:1] == ["--split"]:
        return split(a[1], int(a[2]), int(a[3]))
    out = a[a.index("--out") + 1] if "--out" in a else os.path.join(ROOT, "profiles", "makematrix_wallclock.txt")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    emit("# tools/makematrix_wallclock.py: -makematrix on one MI355X (float); every figure is one run after a warm-up")
    if "--no-reference" not in a:
        if os.path.exists(REFBIN):
            for kind, n, L in COMPARE:
                compare(kind, n, L, emit)
        else:
            emit("reference binary not present: its -makematrix wall time was not measured")
    if "--no-large" not in a:
        for kind, n, L in LARGE:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--split", kind, str(n), str(L)], stdout=subprocess.PIPE,
                                 stderr=subprocess.PIPE, timeout=420)
            if res.returncode != 0:
                emit("FAILED (exit %d) at %s %d x %d: %s" % (res.returncode, kind, n, L, res.stderr.decode()[-2000:]))
                return 1
            emit(res.stdout.decode().strip())
    return 0


if __name__ == "__main__":
    sys.exit(main())
