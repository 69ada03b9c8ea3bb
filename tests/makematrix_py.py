"""TEST INFRASTRUCTURE: the reference's `-makematrix` (printDistances, NJ.tcc:274-288) restated in plain numpy.

For every ordered pair (i, j) of the alignment's rows, diagonal included, codes1 = i:
  1. seqDist (NJ.tcc:1601-1624) on the codes: nUse = columns where both hold a code; without a matrix top = (double) the number
     of those where the codes differ; with the matrix top is a double that accumulates distances[c_i][c_j] (a numeric_t) in
     column order.
  2. dist = (numeric_t)(nUse > 0 ? top / (double) nUse : 1.0)               - Besthit::dist is a numeric_t
  3. unless -rawdist: dist = (numeric_t) logCorrect((double) dist)           - NJ.tcc:322-330, double arithmetic, libm's log
  4. the entry is dist <= 0 ? 0.0 : dist, printed with " %f"; a row is the name, the n entries and a newline.
math.log is libm's log.  The two narrowings are the explicit casts to `dt` below.  The product's version is a pair of device
kernels (veryfasttree_amd/csrc/vft_kernels_seqmatrix.h) and a host formatter (veryfasttree_amd/host/SeqMatrix.h).
"""
import math

import numpy as np

NOCODE = 127


def blosum45_distances(dt):
    """distances[20][20] of the default protein matrix as numeric_t (pinned to the reference's by tests/test_abi_cpu.py)"""
    from veryfasttree_amd import backend
    return backend.distance_tables(None, dt)["distances"].astype(dt)


def log_correct(dist, scoredist):
    """NJ.tcc:322-330 on one double"""
    maxscore = 3.0
    if not scoredist:
        dist = -0.75 * math.log(1.0 - dist * 4.0 / 3.0) if dist < 0.74 else maxscore
    else:
        dist = -1.3 * math.log(1.0 - dist) if dist < 0.99 else maxscore
    return dist if dist < maxscore else maxscore


def matrix(codes, dt, log_corrected=True, distances=None):
    """The n x n entries (step 4's numbers) as an array of dt.  distances: the numeric_t table (proteins), None for %-different."""
    codes = np.asarray(codes, np.uint8)
    dt = np.dtype(dt)
    n, L = codes.shape
    present = codes != NOCODE
    n_use = np.zeros((n, n), np.int64)
    top = np.zeros((n, n), np.float64)
    safe = np.where(present, codes, 0).astype(np.int64)
    for p in range(L):   # column order: what the double accumulator of the matrix branch sees
        both = present[:, p][:, None] & present[:, p][None, :]
        n_use += both
        if distances is None:
            top += both & (codes[:, p][:, None] != codes[:, p][None, :])
        else:
            piece = np.asarray(distances, dt)[safe[:, p][:, None], safe[:, p][None, :]].astype(np.float64)
            top = np.where(both, top + piece, top)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(n_use > 0, top / n_use.astype(np.float64), 1.0).astype(dt)          # first narrowing
    if log_corrected:
        flat = [log_correct(float(x), distances is not None) for x in dist.ravel()]
        dist = np.array(flat, np.float64).reshape(n, n).astype(dt)                           # second narrowing
    return np.where(dist <= 0, dt.type(0), dist).astype(dt)


def text(names, m):
    """the reference's standard output for the entries m"""
    rows = []
    for name, row in zip(names, m):
        rows.append(name + "".join(" %f" % float(x) for x in row) + "\n")
    return "".join(rows).encode()


def fixture_case(d):
    """(codes, names, n_codes, dtype, rawdist) of a tests/golden/mm_*.npz"""
    flags = bytes(d["flags"]).decode().split()
    names = bytes(d["names"]).decode().split("\n")
    return d["codes"], names, 4 if "-nt" in flags else 20, np.float64 if "-double-precision" in flags else np.float32, "-rawdist" in flags


def fixture_matrix(d, log_corrected=None, dt=None):
    codes, names, n_codes, fdt, rawdist = fixture_case(d)
    dt = fdt if dt is None else dt
    return matrix(codes, dt, (not rawdist) if log_corrected is None else log_corrected, blosum45_distances(dt) if n_codes == 20 else None)
