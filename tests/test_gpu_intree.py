"""`-intree` end to end (vft_nj_options.intree; NJDriver::readTree after host/ReadTree.h): whole runs of the reference started from a given
tree (tools/gen_intree_fixtures.py, `VeryFastTree <flags> -threads T -seed 1 -intree T.nwk`) against this backend with the same text.  The
node numbering of the parse decides device rows and the order of every later walk, so the trees must come out byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["intree_nt_4", "intree_nt_5", "intree_nt_200_me", "intree_nt_200_mllen", "intree_nt_200_full", "intree_nt_300_double_gtr",
            "intree_aa_120_lg", "intree_aa_100_wag_double_mllen", "intree_nt_62_dups_caterpillar", "intree_nt_400_t4"]


def case(name):
    """the fixture, its start tree, and the arguments of nj_newick that spell its flags: kw without the stages (what reads the tree), and
    the stages"""
    d = G.load(name)
    run, make, names = G.reference_run(d)
    flags = G.text(d["flags"]).split()
    assert "-nome" in flags or ("-noml" not in flags and "-mllen" not in flags)
    stages = {key: v for key, v in run.kwargs.items() if key in ("me_nni", "spr", "mllen", "ml_nni", "gtr", "gamma")}
    kw = {key: v for key, v in run.kwargs.items() if key not in stages}
    return d, flags, make, names, kw, stages


def text(d, key):
    return bytes(d[key]).decode().strip()


@pytest.mark.parametrize("name", FIXTURES)
def test_the_tree_as_read_is_the_references_nj_line(name):
    """no lengths, no supports: what the reference logs as `NJ\\t<tree>` straight after readTree - topology, child order, every length zero -
    and no join on record"""
    from veryfasttree_amd.backend import nj_newick, last_join_crcs
    d, _, make, names, kw, _ = case(name)
    tree = nj_newick(make, d["codes"], names, me_lengths=False, n_bootstrap=0, **kw)
    assert tree == text(d, "nj_newick")
    assert last_join_crcs()[1] == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_final_trees_match_the_reference(name):
    """the fixture's flags from the given tree: the tree without supports and the tree with them, byte for byte; for the ML cases the
    TreeLogLk lines, the rates and the site categories as the ml_* tests compare them"""
    d, flags, make, names, kw, stages = case(name)
    want = {key: d[key] for key in ("newick", "newick_support", "loglk", "rates", "ratecat") if key in d}
    G.assert_trees_match_the_reference(name, make, d["codes"], names, dict(kw, **stages), want)


def test_mllen_with_gamma_on_a_given_tree():
    """`-intree T -nome -mllen -gamma`: lengths and SH-like supports on T, then the Gamma(20) rescaling"""
    from veryfasttree_amd.backend import nj_newick, last_gamma
    d, _, make, names, kw, stages = case("intree_nt_200_mllen")
    tree, loglk = nj_newick(make, d["codes"], names, me_lengths=True, n_bootstrap=1000, gamma=True, return_loglk=True, **kw, **stages)
    got, want = last_gamma(), d["gamma"]
    print("Gamma(20) LogLk %.3f alpha %.3f rescale %.3f; reference" % got, list(want))
    assert np.allclose(loglk, d["gamma_loglk"], rtol=1e-4, atol=0)
    assert abs(got[0] - want[0]) <= max(1e-4 * abs(want[0]), 6e-4)            # the reference prints three decimals
    assert abs(got[1] - want[1]) < 6e-4 and abs(got[2] - want[2]) < 6e-4
    assert tree == text(d, "gamma_newick_support")


@pytest.mark.parametrize("name,args", [("intree_nt_200_me", []), ("intree_nt_200_mllen", ["-mllen"]), ("intree_nt_62_dups_caterpillar", ["-full"])])
def test_the_tool_prints_the_same_bytes(tmp_path, name, args):
    """tools/nj_tree.py in.fasta -intree start.nwk in each of its three modes"""
    from veryfasttree_amd import synth
    d = G.load(name)
    fa, nwk = str(tmp_path / "in.fasta"), str(tmp_path / "start.nwk")
    synth.codes_to_fasta(d["codes"], fa, synth.ALPHABET_NT)
    with open(nwk, "wb") as fh:
        fh.write(bytes(d["intree"]))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-intree", nwk] + args, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert res.stdout.decode().strip() == text(d, "newick_support")


def test_refusals_leave_the_context_usable():
    """-intree with -slow, with several ranks, through vft_nj_run, with a malformed tree: an error each, before anything reaches the device -
    and the same context then builds the fixture's tree"""
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd import backend
    d, _, _, names, kw, _ = case("intree_nt_200_me")
    codes = d["codes"]
    ops = HipProfileOps(len(codes), codes.shape[1], 4, np.float32, max_nodes=3 * len(codes))
    make = lambda n, L: ops

    class TwoRanks:   # (never called: the refusal comes first)
        struct = backend._Comm(0, 2, backend._ALLGATHER(lambda user, nbytes, device: 1), None, None, None, 0, None, None, 0)

        def pointer(self):
            import ctypes
            return ctypes.cast(ctypes.pointer(self.struct), ctypes.c_void_p)

    with pytest.raises(backend.VftError, match="-slow"):
        backend.nj_newick(make, codes, names, me_lengths=True, slow=True, **kw)
    with pytest.raises(backend.VftError, match="more than one rank"):
        backend.nj_newick(make, codes, names, me_lengths=True, comm=TwoRanks(), **kw)
    with pytest.raises(backend.VftError, match="vft_nj_run"):
        backend.nj_run(ops, codes, intree=kw["intree"])
    with pytest.raises(backend.VftError, match="not recognized as a sequence name"):
        backend.nj_newick(make, codes, names, me_lengths=True, **dict(kw, intree=kw["intree"].replace("s17:", "nobody:")))
    with pytest.raises(backend.VftError, match="at least 4 unique"):
        backend.nj_newick(make, codes[:3], names[:3], me_lengths=True, intree="(s0,s1,s2);")
    assert backend.nj_newick(make, codes, names, me_lengths=True, n_bootstrap=1000, **kw) == text(d, "newick_support")
    assert backend.last_join_crcs()[1] == 0
