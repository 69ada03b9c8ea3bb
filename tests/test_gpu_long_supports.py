"""Local-bootstrap supports (vft_split_supports) on alignments beyond the 1 706 columns whose six pairs k_split_support holds in LDS:
k_split_support_long takes the pairs of a quartet in passes of 3, 2 or 1.  The sums of a resample are the same sums in the
same order, so everything is checked the strict way: the reference's own trees (tools/gen_longsupport_fixtures.py, `-noml [-nome]` runs of
oracle/_ref/VeryFastTree on 1 707 - 10 224 columns) byte for byte, and the pass kernel FORCED (VFT_DEBUG_SUPPORT_PAIRS) on short fixtures
against the one-pass kernel and the fixture."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VFT_DEBUG_SUPPORT_PAIRS = 17
LSUP = ["lsup_nt_16x1707", "lsup_nt_16x1707_boot100", "lsup_nt_12x3414_double", "lsup_nt_12x5121_me", "lsup_nt_8x10224", "lsup_aa_12x2000",
        "lsup_aa_10x3500_double", "lsup_nt_14x2400_gappy"]


def run_lsup(name, pairs=0, keep=None):
    """the fixture's alignment through nj_newick with the fixture's flags -> (tree, the reference's tree)"""
    from veryfasttree_amd.backend import nj_newick
    d = G.load(name)
    run, make_ops, names = G.reference_run(d)

    def make(n, L):
        ops = make_ops(n, L)
        if pairs:
            ops.debug_option(VFT_DEBUG_SUPPORT_PAIRS, pairs)
        if keep is not None:
            keep.append(ops)
        return ops

    return nj_newick(make, d["codes"], names, me_lengths=True, n_bootstrap=run.n_bootstrap, **run.kwargs), G.text(d["newick_support"])


@pytest.mark.parametrize("name", LSUP)
def test_long_alignments_print_the_references_tree(name):
    """`VeryFastTree [-nt] -noml [-nome] [-double-precision] [-boot 100]` on 1 707 - 10 224 columns: lengths and local supports byte for
    byte.  (Before k_split_support_long: "vft_split_supports: alignment too long (... columns, limit 1706)".)"""
    tree, ref = run_lsup(name)
    strip = lambda t: re.sub(r"\)[0-9.]+:", "):", t)
    assert strip(tree) == strip(ref), "topology or lengths differ"
    assert tree == ref


def short_fixture(name, pairs):
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_newick
    d = G.load(name)
    aa = name == "bb_aa_300"
    dt = np.float64 if name.endswith("_double") else np.float32
    dm = G.load("wb_aa_f32") if aa else None

    def make(n, L):
        ops = HipProfileOps(n, L, 20 if aa else 4, dt, max_nodes=3 * n)
        if aa:
            ops.set_distance_matrix(dm["dmat.distances"], dm["dmat.codefreq"], dm["dmat.eigenval"], dm["dmat.eigentot"])
        ops.debug_option(VFT_DEBUG_SUPPORT_PAIRS, pairs)
        return ops

    names = ["s%d" % k for k in range(len(d["codes"]))]
    tree = nj_newick(make, d["codes"], names, dtype=dt, scoredist=aa, me_lengths=True, n_bootstrap=1000)
    return tree, bytes(d["newick_support"]).decode().strip()


_builtin = {}


# fixtures of tests/test_gpu_nj_driver.py (120 - 150 columns): float, double, proteins with the BLOSUM45 matrix
@pytest.mark.parametrize("name", ["bb_nt_200", "bb_nt_300_double", "bb_aa_300"])
@pytest.mark.parametrize("pairs", [0, 1, 2, 3])
def test_forced_pass_kernel_equals_the_one_pass_kernel_on_short_alignments(name, pairs):
    """pairs = 0 is the built-in choice: at these lengths k_split_support itself, with the fixture's tree (alignments of at most 1 706
    columns keep their kernel); 1, 2, 3 force k_split_support_long with that many pairs per pass: the same text"""
    if name not in _builtin:
        _builtin[name] = short_fixture(name, 0)
    tree, ref = _builtin[name] if pairs == 0 else short_fixture(name, pairs)
    assert tree == ref
    assert tree == _builtin[name][0]


def printed_supports(tree):
    """{frozenset of leaf names under an internal group: its printed support} of a Newick text whose groups carry supports"""
    out, stack, k = {}, [], 0
    while k < len(tree):
        ch = tree[k]
        if ch == "(":
            stack.append(set())
            k += 1
        elif ch == ")":
            group = stack.pop()
            m = re.match(r"\)([0-9.]*)", tree[k:])
            if m.group(1):
                out[frozenset(group)] = m.group(1)
            if stack:
                stack[-1] |= group
            k += len(m.group(0))
        elif ch in ",;":
            k += 1
        elif ch == ":":
            k += len(re.match(r":[0-9.eE+-]+", tree[k:]).group(0))
        else:
            m = re.match(r"[^:,()]+", tree[k:])
            stack[-1].add(m.group(0))
            k += len(m.group(0))
    return out


def knuth_columns(n_boot, n_pos):
    """resampleColumns (NJ.tcc:705-727) from the start of Knuth's generator, as NJDriver::computeSupports draws them"""
    import ctypes as C
    from veryfasttree_amd.backend import load_host_library
    r = np.zeros(n_boot * n_pos, np.float64)
    load_host_library().vft_knuth_stream(r.ctypes.data_as(C.c_void_p), C.c_int64(len(r)))
    return np.clip((r * n_pos).astype(np.int64), 0, n_pos - 1).astype(np.int32).reshape(n_boot, n_pos)


def test_direct_calls_with_1_100_and_1001_resamples():
    """vft_split_supports on the final quartets of lsup_nt_16x1707 (children | sibling, up-profile; the driver leaves every profile on the
    device): 1, 100 and 1 001 resamples - one thread, a part of a wavefront, one more than a block of resamples - give the same supports at
    1, 2 and 3 pairs per pass and by the built-in choice, and 100 resamples give what the reference printed with -boot 100"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_run
    d = G.load("lsup_nt_16x1707")
    codes = d["codes"]
    n, L = codes.shape
    joins, _ = nj_run(HipProfileOps(n, L, 4, np.float32), codes)
    assert len(joins) == n - 3 and np.array_equal(joins[:, 2], np.arange(n, 2 * n - 3))
    root = 2 * n - 3
    parent = np.full(root + 1, root, np.int64)
    child = {}
    for i, j, v in joins:
        parent[i] = parent[j] = v
        child[int(v)] = (int(i), int(j))
    root_child = [v for v in range(root) if parent[v] == root]
    assert len(root_child) == 3
    leaves = {v: frozenset(["s%d" % v]) for v in range(n)}
    for v in range(n, root):
        leaves[v] = leaves[child[v][0]] | leaves[child[v][1]]
    a, b, c, dd = [], [], [], []
    for v in range(n, root):   # setupABCD (NJ.tcc:1942-1975); the up-profile of node p is node p + n (NJDriver.h)
        p = int(parent[v])
        others = [x for x in root_child if x != v] if p == root else [child[p][0] if child[p][1] == v else child[p][1], p + n]
        a.append(child[v][0])
        b.append(child[v][1])
        c.append(others[0])
        dd.append(others[1])
    keep = []
    tree, ref = run_lsup("lsup_nt_16x1707_boot100", keep=keep)   # (the same alignment: its profiles and up-profiles stay on the device)
    assert tree == ref
    ops = keep[0]
    printed = printed_supports(ref)
    for n_boot in (1, 100, 1001):
        col = knuth_columns(n_boot, L)
        got = {}
        for pairs in (0, 1, 2, 3):
            ops.debug_option(VFT_DEBUG_SUPPORT_PAIRS, pairs)
            got[pairs] = ops.split_supports(a, b, c, dd, col)
        ops.debug_option(VFT_DEBUG_SUPPORT_PAIRS, 0)
        for pairs in (1, 2, 3):
            assert np.array_equal(got[pairs], got[0]), (n_boot, pairs)
        assert np.array_equal(got[0] * n_boot, np.round(got[0] * n_boot)) and got[0].min() >= 0 and got[0].max() <= 1
        if n_boot == 100:
            assert {leaves[v]: "%.3f" % s for v, s in zip(range(n, root), got[0])} == printed


def test_longer_than_the_nj_phase_takes_is_refused_with_the_limit():
    """8 x 10 256: refused when the context is created, before any launch, with the limit in the message"""
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.backend import nj_newick, VftError
    codes = synth.random_descent_codes(8, 10256, 4, 0.05, 0.0, 3)
    names = ["s%d" % k for k in range(8)]
    with pytest.raises(VftError, match="limit 10240"):
        nj_newick(lambda n, L: HipProfileOps(n, L, 4, np.float32, max_nodes=3 * n), codes, names, me_lengths=True, n_bootstrap=1000)


def test_forced_pairs_that_do_not_fit_are_refused_with_their_limit():
    """3 pairs per pass hold 3 413 columns: forced on 3 414 the call fails before any launch and names that limit"""
    from veryfasttree_amd.backend import VftError
    with pytest.raises(VftError, match="3414 columns, limit 3413"):
        run_lsup("lsup_nt_12x3414_double", pairs=3)


def test_tool_boot_100_prints_the_references_tree(tmp_path):
    from veryfasttree_amd import synth
    d = G.load("lsup_nt_16x1707_boot100")
    fa = str(tmp_path / "in.fa")
    synth.codes_to_fasta(d["codes"], fa, synth.ALPHABET_NT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-boot", "100"], check=True, stdout=subprocess.PIPE, timeout=300)
    assert res.stdout.decode().strip() == bytes(d["newick_support"]).decode().strip()
