"""`-slow` on the GPU: exhaustive neighbour joining over the device-resident distance matrix (vft_exhaustive_*,
veryfasttree_amd/csrc/vft_kernels_exhaustive.h) against the reference's own `-slow` runs (tests/golden/slow_*.npz, produced by
tools/gen_slow_fixtures.py from `VeryFastTree -slow -threads 1`): the operators against the pair kernels, the join order of
every fixture, the printed trees, `-mllen` on the -slow topology, the command-line tool and the refused combinations.

Sizes: a matrix row is read in chunks of 256 columns per wavefront, four wavefronts (rows) per workgroup; slow_nt_257 is one
column past a chunk, slow_nt_65 one past a quarter chunk, slow_nt_600 / slow_nt_1500 take several chunks and workgroups."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from nj_slow_py import SlowNJDriver
from test_nj_driver_cpu import unique_codes

pytestmark = pytest.mark.gpu

CASES = ["slow_nt_200", "slow_nt_600", "slow_nt_1500", "slow_nt_300_double", "slow_aa_300", "slow_nt_mirror", "slow_nt_mirror_double",
         "slow_nt_5", "slow_nt_4", "slow_nt_65", "slow_nt_257"]


def dtype_of(name):
    return np.float64 if "double" in name else np.float32


def maker(name, big=True):
    """make_ops(n, L) for a fixture: alphabet, precision and - for proteins - the BLOSUM45-derived distance matrix"""
    from veryfasttree_amd import HipProfileOps
    aa = "_aa_" in name
    dm = G.load("wb_aa_f32") if aa else None

    def make(n, L):
        ops = HipProfileOps(n, L, 20 if aa else 4, dtype_of(name), max_nodes=(3 if big else 2) * n)
        if aa:
            ops.set_distance_matrix(dm["dmat.distances"], dm["dmat.codefreq"], dm["dmat.eigenval"], dm["dmat.eigentot"])
        return ops
    return make


class DeviceChecked(SlowNJDriver):
    """the Python -slow driver on the HIP backend, with the device matrix kept beside its own distance table"""
    checked_searches = checked_rows = 0

    def active(self):
        return np.nonzero(self.parent[:self.maxnode] < 0)[0]

    def exhaustive_search(self, n_active):
        if len(self.joins) in (0, 3):
            # the lexicographic arg-min (criterion, i, j) of the pair kernel's own criteria over all active pairs
            act = self.active()
            iu = np.triu_indices(n_active, 1)
            lo, hi = act[iu[0]], act[iu[1]]
            d, _, c = self.ops.setDistCriterion(lo, hi, n_active, 0, self.totdiam)
            k = np.lexsort((hi, lo, c))[0]
            i, j, dist, crit = self.ops.exhaustive_search(n_active)
            assert (i, j) == (int(lo[k]), int(hi[k]))
            assert dist == d[k] and crit == c[k]
            self.checked_searches += 1
        return SlowNJDriver.exhaustive_search(self, n_active)

    def after_join(self, i, j, newnode, n_active):
        self.ops.exhaustive_join(i, j, newnode)
        if len(self.joins) <= 3:
            nodes, dist = self.ops.exhaustive_row(newnode)
            assert sorted(nodes.tolist()) == self.active().tolist()
            others = nodes != newnode
            want = self.ops.blockDistances(nodes[others], [newnode], n_active, 0, self.totdiam)[:, 0]
            assert np.array_equal(dist[others], want)
            self.checked_rows += 1


@pytest.mark.parametrize("name", ["slow_nt_mirror", "slow_nt_mirror_double", "slow_aa_300"])
def test_search_and_new_row_equal_the_pair_kernels(name):
    """After the fill and again after three joins: the search's (i, j, dist, criterion) is the lexicographic arg-min of
    vft_pair_distances over all active pairs, and the newest node's matrix row is vft_block_distances(actives, {newnode}),
    bit for bit."""
    d = G.load(name)
    codes = unique_codes(d["codes"])
    ops = maker(name, big=False)(*codes.shape)
    drv = DeviceChecked(ops, codes)
    ops.exhaustive_create()
    ops.exhaustive_fill()
    joins = drv.run(max_joins=4)
    assert drv.checked_searches == 2 and drv.checked_rows == 3
    assert np.array_equal(np.array([j[:3] for j in joins]), d["joins"][:4])
    ops.close()


@pytest.mark.parametrize("name", CASES)
def test_join_order_matches_the_reference(name):
    """vft_nj_run with slow = 1: every join of the reference's -slow run, and its criteria (printed with %.6f)"""
    from veryfasttree_amd.backend import nj_run
    d = G.load(name)
    codes = unique_codes(d["codes"])
    ops = maker(name, big=False)(*codes.shape)
    joins, crit = nj_run(ops, codes, slow=True)
    want = d["joins"]
    assert len(joins) == len(want) == len(codes) - 3
    bad = np.nonzero((joins != want).any(axis=1))[0]
    assert len(bad) == 0, "first differing join %d: got %s want %s" % (bad[0], joins[bad[0]], want[bad[0]])
    assert np.allclose(crit, d["join_criterion"], atol=1e-6)
    ops.close()


@pytest.mark.parametrize("name", CASES)
def test_trees_equal_the_reference(name):
    """the "NJ" tree, the final tree of -slow -noml -nome -nosupport and the one with local-bootstrap supports, byte for byte"""
    from veryfasttree_amd.backend import nj_newick
    d = G.load(name)
    names = ["s%d" % k for k in range(len(d["codes"]))]
    kw = dict(dtype=dtype_of(name), scoredist="_aa_" in name, slow=True)
    assert nj_newick(maker(name), d["codes"], names, **kw) == bytes(d["nj_newick"]).decode()
    assert nj_newick(maker(name), d["codes"], names, me_lengths=True, **kw) == bytes(d["newick"]).decode().strip()
    assert nj_newick(maker(name), d["codes"], names, me_lengths=True, n_bootstrap=1000, **kw) == bytes(d["newick_support"]).decode().strip()


def test_mllen_on_the_slow_topology():
    """`-slow -nome -mllen -nocat`: TreeLogLk of every round and the tree, as tests/test_gpu_ml_lengths.py compares the ml_*
    fixtures; then the default SH-like supports"""
    from veryfasttree_amd.backend import nj_newick
    name = "slow_mllen_nt_200"
    d = G.load(name)
    names = ["s%d" % k for k in range(len(d["codes"]))]
    tree, loglk = nj_newick(maker(name), d["codes"], names, me_lengths=True, mllen=True, return_loglk=True, slow=True)
    want = d["loglk"]
    assert len(loglk) == len(want)
    assert np.allclose(loglk, want, rtol=1e-4, atol=0)
    assert np.allclose(loglk, want, rtol=0, atol=6e-5), (loglk, want)   # printed with %.4f
    ref = bytes(d["newick"]).decode().strip()
    strip = lambda t: re.sub(r":[0-9.eE+-]+", ":", t)
    assert strip(tree) == strip(ref)
    got_len = np.array([float(x) for x in re.findall(r":([0-9.eE+-]+)", tree)])
    ref_len = np.array([float(x) for x in re.findall(r":([0-9.eE+-]+)", ref)])
    assert np.allclose(got_len, ref_len, rtol=5e-3, atol=2e-5)
    assert tree == ref, "lengths differing in the printed digits: %d of %d" % (int((got_len != ref_len).sum()), len(ref_len))
    boot = nj_newick(maker(name), d["codes"], names, me_lengths=True, mllen=True, n_bootstrap=1000, slow=True)
    ref = bytes(d["newick_support"]).decode().strip()
    strip = lambda t: re.sub(r"\)[0-9.]+:", "):", t)
    assert strip(boot) == strip(ref)
    got = np.array([float(x) for x in re.findall(r"\)([0-9.]+):", boot)])
    want = np.array([float(x) for x in re.findall(r"\)([0-9.]+):", ref)])
    assert len(got) == len(want) and np.abs(got - want).max() <= 0.002 + 1e-9 and (got != want).mean() <= 0.05


def test_tool_prints_the_reference_tree():
    """tools/nj_tree.py -slow on the FASTA of bb_nt_200 (slow_nt_200's alignment) prints what `VeryFastTree -nt -slow -noml -nome` printed"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fa = os.path.join(root, "tests", "golden", "bb_nt_200.fa")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "nj_tree.py"), fa, "-slow"], check=True, stdout=subprocess.PIPE,
                         timeout=300).stdout.decode().strip()
    assert out == bytes(G.load("slow_nt_200")["newick_support"]).decode().strip()
    for flags in (["-slow", "-fastest"], ["-slow", "-full"]):
        res = subprocess.run([sys.executable, os.path.join(root, "tools", "nj_tree.py"), fa] + flags, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, timeout=300)
        assert res.returncode != 0 and b"-slow" in res.stderr and not res.stdout


def test_default_path_is_unchanged():
    """slow = 0 on the same alignment still gives bb_nt_200's joins"""
    from veryfasttree_amd.backend import nj_run
    d = G.load("bb_nt_200")
    codes = unique_codes(d["codes"])
    joins, _ = nj_run(maker("bb_nt_200", big=False)(*codes.shape), codes, slow=False)
    assert np.array_equal(joins, d["joins"])
    assert not np.array_equal(joins, G.load("slow_nt_200")["joins"])


def test_rejected_combinations():
    """-slow with -fastest, with the NNI / SPR stages or with several ranks is an error with a message, not another algorithm"""
    from veryfasttree_amd import VftError
    from veryfasttree_amd.backend import _ALLGATHER, _Comm, nj_newick, nj_run
    d = G.load("slow_nt_5")
    codes = d["codes"]
    names = ["s%d" % k for k in range(len(codes))]
    make = maker("slow_nt_5")
    with pytest.raises(VftError, match="-fastest"):
        nj_run(make(*codes.shape), codes, slow=True, fastest=True)
    for kw in (dict(me_nni=True), dict(me_nni=True, spr=2), dict(ml_nni=20)):
        with pytest.raises(VftError, match="not built"):
            nj_newick(make, codes, names, me_lengths=True, slow=True, **kw)

    class TwoRanks:
        struct = _Comm(0, 2, _ALLGATHER(), None, None, None, 0, None, None, 0)

        def pointer(self):
            return C.cast(C.pointer(self.struct), C.c_void_p)

    with pytest.raises(VftError, match="more than one rank"):
        nj_run(make(*codes.shape), codes, slow=True, comm=TwoRanks())


def test_search_needs_current_out_distances():
    """the search refuses out-distances that do not carry the stamp n_active instead of rescaling them silently"""
    from veryfasttree_amd import VftError
    d = G.load("slow_nt_5")
    codes = d["codes"]
    ops = maker("slow_nt_5", big=False)(*codes.shape)
    SlowNJDriver(ops, codes)   # the constructor's state: every leaf's out-distance computed for n_active = 5
    ops.exhaustive_create()
    ops.exhaustive_fill()
    assert ops.exhaustive_search(5)[:2] == tuple(int(x) for x in d["joins"][0][:2])
    with pytest.raises(VftError, match="n_active"):
        ops.exhaustive_search(4)
    ops.set_out_distances(2, np.zeros(1, np.float32), np.array([50]))
    with pytest.raises(VftError, match="not current"):
        ops.exhaustive_search(5)
    ops.close()
