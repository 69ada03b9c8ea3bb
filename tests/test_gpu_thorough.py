"""The thorough search on the device and end to end: `-mlacc N`, `-slownni`, `-nni N`, `-mlnni N`, `-sprlength N`
(vft_nj_options.ml_accuracy ... spr_length).

Whole runs of the reference with these options (tools/gen_thorough_fixtures.py) against nj_newick with the new keyword arguments, byte
for byte: the tree without supports, the tree with supports, the TreeLogLk lines to the printed digit.  These runs are the first to enter
the ml_accuracy >= 2 branches of k_ml_quartet (three or more rounds per quartet, no alternative dropped), of its long-alignment twin
(thor_nt_30_x2200), of the whole-column protein instance (thor_aa_24_x600_lg) and of k_ml_nni_decide, the always-second-pass mode of the
split tests, and walks in which no subtree is skipped.  thor_nt_300_chains has SPR chains beyond the default's ten steps (`-sprlength 30`
and 64 move its topology); thor_nt_150_mllen is `-nome -mllen` with `-mlacc` (the supports' second pass, three rounds of the -gtr fit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"thor_nt_150": 8, "thor_nt_60_gtr": 2, "thor_aa_60_lg": 3, "thor_aa_40_wag_double": 2, "thor_nt_400_noisy": 5,
            "thor_aa_150_noisy": 1, "thor_nt_30_x2200": 1, "thor_aa_24_x600_lg": 1, "thor_nt_300_chains": 2, "thor_nt_150_mllen": 2}   # name: runs
RUNS = [(name, k) for name, n in FIXTURES.items() for k in range(n)]


def case(name, k):
    """run k of a fixture as the arguments of nj_newick"""
    d = G.load(name)
    pre = "r%d_" % k
    run, make, names = G.reference_run(d, pre)
    want = {key: d[pre + key] for key in ("newick", "newick_support", "loglk", "rates", "ratecat") if pre + key in d}
    return d, G.text(d[pre + "flags"]).split(), make, names, run.kwargs, want


text = G.text


@pytest.mark.parametrize("name,k", RUNS)
def test_trees_match_the_reference(name, k):
    """the run's flags, without and with supports, byte for byte; the ML runs add the TreeLogLk lines, the rates and the site categories as
    the ml_* / pseudo tests compare them"""
    d, flags, make, names, kw, want = case(name, k)
    G.assert_trees_match_the_reference("%s %d" % (name, k), make, d["codes"], names, kw, want)


def test_the_tool_runs_the_accuracy_recipe(tmp_path):
    """tools/nj_tree.py as a child process: thor_nt_150 with `-full -spr 4 -mlacc 2 -slownni`"""
    from veryfasttree_amd import synth
    d, flags, _, _, _, want = case("thor_nt_150", 3)
    assert flags == ["-nt", "-spr", "4", "-mlacc", "2", "-slownni"]
    fa = str(tmp_path / "thor_nt_150.fa")
    synth.codes_to_fasta(d["codes"], fa, synth.ALPHABET_NT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-full", "-spr", "4", "-mlacc", "2", "-slownni"], check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    got = res.stdout.decode().strip()
    ref = text(want["newick_support"])
    assert got == ref
    ll = [float(l.split("\t")[2]) for l in res.stderr.decode().splitlines() if l.startswith("TreeLogLk")]
    assert np.allclose(ll, want["loglk"], rtol=0, atol=6e-5)


def test_the_tool_takes_the_accuracy_with_mllen(tmp_path):
    """`-mllen -mlacc 2` through tools/nj_tree.py: the reference's supports, and the TreeLogLk lines keep the label of a -mllen run"""
    from veryfasttree_amd import synth
    d, flags, _, _, _, want = case("thor_nt_150_mllen", 0)
    assert flags == ["-nt", "-nome", "-mllen", "-mlacc", "2"]
    fa = str(tmp_path / "thor_nt_150.fa")
    synth.codes_to_fasta(d["codes"], fa, synth.ALPHABET_NT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-mllen", "-mlacc", "2"], check=True,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.stdout.decode().strip() == text(want["newick_support"])
    lines = [l for l in res.stderr.decode().splitlines() if l.startswith("TreeLogLk")]
    assert [l.split("\t")[1] for l in lines] == ["Length%d" % (k + 1) for k in range(len(want["loglk"]))]
    assert np.allclose([float(l.split("\t")[2]) for l in lines], want["loglk"], rtol=0, atol=6e-5)


@pytest.mark.parametrize("name,aa", [("full_nt_200", None), ("full_aa_150_lg", "lg")])
def test_zeroed_members_move_nothing(name, aa):
    """all five members at 0 - what a caller compiled against the shorter struct's meaning hands over - give the default pipeline's tree"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_newick
    d = G.load(name)
    names = ["s%d" % i for i in range(len(d["codes"]))]
    make = lambda n, L: HipProfileOps(n, L, 20 if aa else 4, np.float32, max_nodes=3 * n)
    kw = dict(dtype=np.float32, me_lengths=True, me_nni=True, spr=2, ml_nni=20, ml_accuracy=0, slow_nni=False, nni_rounds=None, ml_nni_rounds=None,
              spr_length=None)
    if aa:
        kw["aa_model"] = aa
    tree, loglk = nj_newick(make, d["codes"], names, return_loglk=True, **kw)
    assert len(loglk) == len(d["loglk"]) and np.allclose(loglk, d["loglk"], rtol=0, atol=6e-5)
    assert tree == text(d["newick"])
    assert nj_newick(make, d["codes"], names, n_bootstrap=1000, **kw) == text(d["newick_support"])


def test_refusals_with_a_device():
    """the same refusals a caller meets with a context in hand: nothing has been uploaded when they come"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import nj_newick, VftError
    d = G.load("thor_aa_150_noisy")
    names = ["s%d" % i for i in range(len(d["codes"]))]
    make = lambda n, L: HipProfileOps(n, L, 20, np.float32, max_nodes=3 * n)
    kw = dict(me_lengths=True, me_nni=True, spr=2, aa_model="jtt")
    with pytest.raises(VftError, match=r"spr_length \(-sprlength\) is above 64: the chain buffers of MLLengths::sprAttempt hold 64 steps"):
        nj_newick(make, d["codes"], names, spr_length=65, **kw)
    for key in ("ml_accuracy", "slow_nni", "nni_rounds", "ml_nni_rounds", "spr_length"):
        with pytest.raises(VftError, match=r"vft_nj_options\.%s \(-\w+\) is negative" % key):
            nj_newick(make, d["codes"], names, **dict(kw, **{key: -1}))
    # 64 is taken
    assert nj_newick(make, d["codes"], names, spr_length=64, **kw).endswith(";")
