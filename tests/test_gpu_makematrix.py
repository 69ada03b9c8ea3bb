"""`-makematrix` on the GPU: the all-pairs kernels (vft_seq_matrix_rows, veryfasttree_amd/csrc/vft_kernels_seqmatrix.h), the slab
driver (vft_nj_make_matrix, veryfasttree_amd/host/SeqMatrix.h) and the command-line tool against the reference's own output
(tests/golden/mm_*.npz, tools/gen_makematrix_fixtures.py) and against the numpy restatement that tests/test_makematrix_cpu.py pins
to that output byte for byte.

Sizes: a lane owns a column sequence (64 per tile), a wavefront 16 row sequences, a workgroup 64; codes come in chunks of 16
columns.  130 x 75 = two full tiles and a partial one, two row blocks and a partial one, four chunks and a partial one; 65 x 17 is
one past a tile and one past a chunk; 2 x 1 the smallest.  Numbers are compared bit for bit: the kernels' arithmetic is the
reference's (integer counts or an ordered double sum, one division, glibc's log restated), so there is no tolerance to state."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import golden_util as G
import makematrix_py as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["mm_nt_130x75", "mm_nt_130x75_double", "mm_nt_130x75_raw", "mm_aa_130x75", "mm_aa_130x75_double", "mm_aa_130x75_raw",
         "mm_nt_65x17", "mm_nt_2x1", "mm_aa_70x33"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


@functools.lru_cache(maxsize=None)
def expected(name, log_corrected):
    """the restatement's numbers in the fixture's precision (computed once per case; callers do not modify them)"""
    m = M.fixture_matrix(fixture(name), log_corrected=log_corrected)
    m.setflags(write=False)
    return m


def make_ops(name, with_matrix=None):
    from veryfasttree_amd import HipProfileOps, backend
    codes, _, n_codes, dt, _ = M.fixture_case(fixture(name))
    ops = HipProfileOps(codes.shape[0], codes.shape[1], n_codes, dt, max_nodes=codes.shape[0])   # max_nodes == n_seqs is enough
    ops.upload_leaves(codes)
    if (n_codes == 20) if with_matrix is None else with_matrix:
        t = backend.distance_tables(None, dt)
        ops.set_distance_matrix(t["distances"], t["codefreq"], t["eigenval"], t["eigentot"])
    return ops


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def full_matrix(name, log_corrected):
    ops = make_ops(name)
    n = ops.n_seqs
    got = ops.seq_matrix_rows(0, n, log_correct=log_corrected).copy()
    ops.close()
    got.setflags(write=False)
    return got


@pytest.mark.parametrize("log_corrected", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_matrix_equals_the_restatement_bit_for_bit(name, log_corrected):
    got, want = full_matrix(name, log_corrected), expected(name, log_corrected)
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%d entries differ, first (%d, %d): got %r want %r" % (len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", ["mm_nt_130x75", "mm_aa_130x75"])
def test_row_slabs_equal_the_rows_of_the_full_call(name):
    full = full_matrix(name, True)
    ops = make_ops(name)
    for r0, r1 in ((37, 101), (0, 1), (129, 130), (64, 128)):
        got = ops.seq_matrix_rows(r0, r1)
        assert got.shape == (r1 - r0, 130)
        assert np.array_equal(bits(got), bits(full[r0:r1])), (r0, r1)
    ops.close()


@pytest.mark.parametrize("name", ["mm_nt_130x75", "mm_aa_130x75_double"])
def test_padding_columns_of_a_wider_stride_are_left_alone(name):
    ops = make_ops(name)
    n = ops.n_seqs
    buf = np.full((n, n + 3), -7.25, ops.dt)
    got = ops.seq_matrix_rows(0, n, ld=n + 3, out=buf)
    assert np.array_equal(bits(got), bits(full_matrix(name, True)))
    assert (buf[:, n:] == -7.25).all()
    ops.close()


@pytest.mark.parametrize("slab_rows", [1, 7, 64, None])
@pytest.mark.parametrize("name", ["mm_nt_130x75", "mm_aa_130x75_double", "mm_nt_2x1"])
def test_make_matrix_writes_the_reference_text(name, slab_rows):
    from veryfasttree_amd import backend
    d = fixture(name)
    codes, names, n_codes, dt, rawdist = M.fixture_case(d)
    with tempfile.TemporaryFile() as fh:
        backend.make_matrix(codes, names, n_codes, dt, rawdist, fh.fileno(), slab_rows=slab_rows)
        fh.seek(0)
        got = fh.read()
    assert got == bytes(d["text"])


def test_make_matrix_reports_its_slabs():
    from veryfasttree_amd import backend
    codes, names, n_codes, dt, rawdist = M.fixture_case(fixture("mm_nt_130x75"))
    with tempfile.TemporaryFile() as fh:
        t = backend.make_matrix(codes, names, n_codes, dt, rawdist, fh.fileno(), slab_rows=7, return_times=True)
    assert (t["slabs"], t["slab_rows"], t["bytes"]) == (19, 7, len(bytes(fixture("mm_nt_130x75")["text"])))


def tool_flags(name):
    _, _, n_codes, dt, rawdist = M.fixture_case(fixture(name))
    return (["-aa"] if n_codes == 20 else []) + (["-double"] if dt == np.float64 else []) + (["-rawdist"] if rawdist else [])


@pytest.mark.parametrize("name", CASES)
def test_tool_prints_the_reference_text(name, tmp_path):
    from veryfasttree_amd import synth
    d = fixture(name)
    codes, names, n_codes, _, _ = M.fixture_case(d)
    fa = str(tmp_path / (name + ".fa"))
    synth.codes_to_fasta(codes, fa, synth.ALPHABET_AA if n_codes == 20 else synth.ALPHABET_NT)   # names s0, s1, ... as in the fixture
    assert names == ["s%d" % k for k in range(len(codes))]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), "-makematrix"] + tool_flags(name) + [fa],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()
    assert res.stdout == bytes(d["text"])


def test_refusals(tmp_path):
    from veryfasttree_amd import VftError, backend, synth
    # a nucleotide context with a distance matrix set
    ops = make_ops("mm_nt_65x17")
    z = np.zeros((4, 4))
    ops.set_distance_matrix(z, z, np.zeros(4), np.zeros(4))
    with pytest.raises(VftError, match="distance matrix"):
        ops.seq_matrix_rows(0, 65)
    ops.close()
    # proteins without one
    ops = make_ops("mm_aa_70x33", with_matrix=False)
    with pytest.raises(VftError, match="distance matrix"):
        ops.seq_matrix_rows(0, 70)
    ops.close()
    # rows beyond the alignment, an empty range
    ops = make_ops("mm_nt_65x17")
    for r0, r1 in ((0, 66), (64, 66), (5, 5), (-1, 3)):
        with pytest.raises(VftError, match="rows"):
            ops.seq_matrix_rows(r0, r1)
    assert np.array_equal(bits(ops.seq_matrix_rows(0, 65)), bits(full_matrix("mm_nt_65x17", True)))   # the context is still good
    ops.close()
    # duplicate names
    codes, names, n_codes, dt, rawdist = M.fixture_case(fixture("mm_nt_65x17"))
    with tempfile.TemporaryFile() as fh:
        with pytest.raises(VftError, match="Non-unique name"):
            backend.make_matrix(codes, names[:-1] + [names[3]], n_codes, dt, rawdist, fh.fileno())
        fh.seek(0)
        assert fh.read() == b""
    # the tool: -makematrix with a tree option
    fa = str(tmp_path / "a.fa")
    synth.codes_to_fasta(codes, fa)
    for extra in (["-slow"], ["-fastest"], ["-mllen"], ["-full"]):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), "-makematrix", fa] + extra, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=120)
        assert res.returncode != 0 and res.stdout == b"" and b"-makematrix" in res.stderr and extra[0].encode() in res.stderr


def test_more_than_one_rank_is_refused():
    import ctypes as C
    from veryfasttree_amd import VftError, backend
    codes, names, n_codes, dt, rawdist = M.fixture_case(fixture("mm_nt_2x1"))

    class TwoRanks:
        struct = backend._Comm(0, 2, backend._ALLGATHER(lambda u, n, d: 1), None, None, None, 0, None, None, 0)

        def pointer(self):
            return C.cast(C.pointer(self.struct), C.c_void_p)

    with tempfile.TemporaryFile() as fh:
        with pytest.raises(VftError, match="one GPU"):
            backend.make_matrix(codes, names, n_codes, dt, rawdist, fh.fileno(), comm=TwoRanks())


def sweep_hits(ops, codes, matrix_calls):
    """smoke()'s sweep: seed 5 against everything, 40 hits"""
    n = len(codes)
    if matrix_calls:
        ops.seq_matrix_rows(0, n)
    ops.set_node_scalars(0, np.zeros(n, np.float32), (codes != 127).sum(1).astype(np.float32), np.zeros(n, np.float32))
    ops.outProfile(np.arange(n))
    ops.set_out_distances(0, np.zeros(n, np.float32), np.full(n, 10 * n))
    ops.setOutDistance(None, n, 0.0)
    if matrix_calls:
        ops.seq_matrix_rows(3, 77, log_correct=False)
    return ops.setBestHit(5, n, int(n * 0.01), 0.0, 40)


def test_matrix_calls_leave_the_arena_alone():
    """self-check: a sweep after matrix calls returns what it returns on a fresh context"""
    from veryfasttree_amd import HipProfileOps, synth
    codes = synth.random_descent_codes(300, 120, 4, 0.05, 0.03, seed=7)   # smoke()'s alignment
    res = []
    for matrix_calls in (False, True):
        ops = HipProfileOps(codes.shape[0], codes.shape[1], 4, np.float32)
        ops.upload_leaves(codes)
        res.append(sweep_hits(ops, codes, matrix_calls))
        ops.close()
    (h0, b0), (h1, b1) = res
    assert b0 == b1 and h0.tobytes() == h1.tobytes()
