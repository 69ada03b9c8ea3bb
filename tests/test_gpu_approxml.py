"""`-approxml` on the device: the two posterior operators against the numpy restatement (tests/approx_posterior_np.py, anchored on the CPU
oracle by tests/test_approxml_cpu.py), the chain kernel against plain calls, whole runs against the reference's bytes
(tests/golden/approx_aa_*.npz, tools/gen_approxml_fixtures.py) and the state handling of the two new setters."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import approx_posterior_np as R
import golden_util as G
from oracle import tolerances

pytestmark = pytest.mark.gpu

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G.GOLDEN, "approx_aa_*.npz")))
I64, I32, P = C.c_int64, C.c_int32, C.c_void_p


def ptr(a):
    return a.ctypes.data_as(P)


def same(p, q):
    (w1, c1, f1), (w2, c2, f2) = p, q
    vec = (w1 > 0) & (c1 == 127)
    return np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(c1, c2) and np.array_equal(f1[vec].view(np.uint8), f2[vec].view(np.uint8))


_cases = {}


def case_of(dt):
    """the shared operator case and the restatement's answers, computed once per precision and left alone"""
    dt = np.dtype(dt)
    if dt not in _cases:
        from veryfasttree_amd import backend
        t = backend.aa_model_tables("lg", dt)
        n = backend.aa_near_tables("lg", dt)
        near = (n["nearP"], n["nearFreq"])
        c = R.operator_case(t, dt)
        exact, _ = R.run_case(c, t, dt, None, tolerances(dt))
        rough, notes = R.run_case(c, t, dt, near, tolerances(dt))
        _cases[dt] = dict(t=t, near=near, c=c, exact=exact, rough=rough, notes=notes)
    return _cases[dt]


def make_ops(dt, k, rows):
    """a context with the case's leaves, the uploaded profile, LG and its near-constant tables; rows: the ML stage's layout, where the
    posteriors of proteins run through k_posterior_quad (otherwise the whole-column kernel, stash and tile commit)"""
    from veryfasttree_amd import HipProfileOps
    ops = HipProfileOps(R.N_SEQS, R.N_POS, 20, dt, max_nodes=R.MAX_NODES)
    ops.upload_leaves(k["c"]["codes"])
    ops.profile_upload(R.CUSTOM, k["c"]["custom"])
    ops.set_max_node(R.MAX_NODES)
    if rows:
        ops.set_profile_rows(True)
    ops.set_rates(np.array(R.RATES, dt), k["c"]["ratecat"])
    ops.set_ml_limits(*tolerances(dt))
    t = k["t"]
    ops.set_transition_matrix(t["stat"], t["statinv"], t["eigenval"], t["codefreq"], t["eigeninv"], t["eigeninvT"])
    ops.set_near_posteriors(*k["near"])
    return ops


@pytest.mark.parametrize("rows", [False, True], ids=["whole_column", "quad"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_posterior_operators_equal_the_restatement(dt, rows):
    """5 posteriors x 70 columns (3 of them read the outputs of the first call), branch lengths 0.01 / 0.1 / 1.0, two rate categories:
    with the switch on weights, codes and vectors equal the restatement's, with it off they are today's exact result - including the
    column whose dominant state sits on lane 3 of its quad while another lane's state fails the ratio test."""
    k = case_of(dt)
    # asked of the restatement before the device is: both outcomes occur, and the quad kernels' hard column
    for node in R.SECOND:
        what = k["notes"][node][0]
        assert (what == R.ROUGH).any() and ((what == R.GAVE_UP) | (what == R.NEVER)).any()
    what, ch, fail = k["notes"][9]
    assert ((what == R.GAVE_UP) & (ch % 4 == 3) & (fail % 4 != 3)).any()
    ops = make_ops(dt, k, rows)
    try:
        for on, want in ((True, k["rough"]), (False, k["exact"]), (True, k["rough"])):
            ops.set_approx_ml(on)
            assert ops.get_approx_ml() == on
            for call in k["c"]["calls"]:
                out, a, b, l1, l2 = (list(x) for x in zip(*call))
                ops.posteriorProfile(out, a, b, l1, l2)
                for node in out:
                    got = ops.profile_download(node)
                    assert np.array_equal(got[0], want[node][0]) and np.array_equal(got[1], want[node][1]), (on, node)
                    assert np.array_equal(got[2], want[node][2]), (on, node, np.argwhere(got[2] != want[node][2])[:5])
    finally:
        ops.close()


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_chain_equals_plain_calls(dt):
    """vft_posterior_chain_blen over a node and then its parent (k_posterior_chain: a thread owns the column) with the switch on equals
    two plain calls (k_posterior_quad) - and the restatement"""
    k = case_of(dt)
    ops = make_ops(dt, k, True)
    try:
        ops.set_approx_ml(True)
        bl = np.zeros(R.MAX_NODES, dt)
        bl[[0, 1, 2, 11, 13]] = [0.01, 0.1, 0.3, 0.05, 0.05]
        ops.branch_lengths_set(0, bl)
        out, a, b = np.array([11, 12], np.int64), np.array([0, 11], np.int64), np.array([1, 2], np.int64)
        assert ops.lib.vft_posterior_chain_blen(ops.ctx, I32(2), ptr(out), ptr(a), ptr(b), ptr(a.copy()), ptr(b.copy())) == 0
        ops.posteriorProfileBlen([13], [0], [1], [0], [1])
        ops.posteriorProfileBlen([14], [13], [2], [13], [2])
        assert same(ops.profile_download(11), ops.profile_download(13))
        assert same(ops.profile_download(12), ops.profile_download(14))
        profs = {i: ((k["c"]["codes"][i] != 127).astype(dt), k["c"]["codes"][i], np.zeros((R.N_POS, 20), dt)) for i in range(3)}
        rates, rc, lim = np.array(R.RATES, dt), k["c"]["ratecat"], tolerances(dt)
        n11, what11, _, _ = R.posterior(profs[0], profs[1], float(bl[0]), float(bl[1]), rates, rc, k["t"], k["near"], lim[0], lim[1])
        n12, what12, _, _ = R.posterior(n11, profs[2], float(bl[11]), float(bl[2]), rates, rc, k["t"], k["near"], lim[0], lim[1])
        assert (what11 == R.ROUGH).any() and (what12 == R.ROUGH).any() and (what12 != R.ROUGH).any()
        assert same(ops.profile_download(11), n11) and same(ops.profile_download(12), n12)
    finally:
        ops.close()


def run_fixture(name, approx):
    d = G.load(name)
    flags = G.text(d["flags"]).split()
    if not approx:
        d = dict(d, flags=np.frombuffer(" ".join(f for f in flags if f != "-approxml").encode(), np.uint8))
    run, make, names = G.reference_run(d)
    assert run.kwargs.get("approx_ml", False) == approx
    made = []

    def make_and_keep(n, L):
        ops = make(n, L)
        made.append(ops)
        return ops
    return d, run, make_and_keep, names, made


@pytest.mark.parametrize("name", FIXTURES)
def test_whole_runs_print_the_references_bytes(name):
    """`VeryFastTree <flags> -approxml -threads 1` through refflags -> nj_newick: the TreeLogLk lines to the printed digit, the tree
    and the tree with supports byte for byte"""
    d, run, make, names, made = run_fixture(name, True)
    want = {key: d[key] for key in ("newick", "newick_support", "loglk", "rates", "ratecat")}
    G.assert_trees_match_the_reference(name, make, d["codes"], names, run.kwargs, want, n_bootstrap=run.n_bootstrap)
    assert all(ops.get_approx_ml() for ops in made)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_same_command_without_the_flag_is_the_control(name):
    from veryfasttree_amd.backend import nj_newick
    d, run, make, names, made = run_fixture(name, False)
    tree = nj_newick(make, d["codes"], names, me_lengths=True, **run.kwargs)
    assert tree == G.text(d["control_newick"])
    assert tree != G.text(d["newick"])
    assert not any(ops.get_approx_ml() for ops in made)


def test_the_long_alignment_reaches_the_workspace_kernels():
    """2 200 columns is beyond every register-resident instance of the line-search kernels (4 x 512 columns for proteins): the
    posteriors inside k_ml_node_lengths_long / k_ml_quartet_long take the approximate branch too"""
    d = G.load("approx_aa_lg_12_long")
    assert d["codes"].shape[1] > 4 * 512


def test_the_switch_without_tables_fails_and_says_what_is_missing():
    dt = np.float32
    k = case_of(dt)
    from veryfasttree_amd import VftError
    ops = make_ops(dt, k, True)
    try:
        ops.set_approx_ml(True)
        call = k["c"]["calls"][0]
        out, a, b, l1, l2 = (list(x) for x in zip(*call))
        ops.posteriorProfile(out, a, b, l1, l2)                     # tables present: runs
        t = k["t"]
        ops.set_transition_matrix(t["stat"], t["statinv"], t["eigenval"], t["codefreq"], t["eigeninv"], t["eigeninvT"])   # ... clears them
        for attempt in (lambda: ops.posteriorProfile(out, a, b, l1, l2), lambda: ops.posteriorProfileBlen(out, a, b, a, b)):
            with pytest.raises(VftError, match="vft_set_near_posteriors"):
                attempt()
        ops.set_approx_ml(False)                                     # exact needs no tables
        ops.posteriorProfile(out, a, b, l1, l2)
        assert same(ops.profile_download(out[0]), k["exact"][out[0]])
        ops.set_approx_ml(True)
        ops.set_near_posteriors(*k["near"])
        ops.posteriorProfile(out, a, b, l1, l2)
        assert same(ops.profile_download(out[0]), k["rough"][out[0]])
    finally:
        ops.close()


def test_four_states_accept_the_switch_and_ignore_it():
    """a 4-state context refuses the tables, takes the switch, and prints a `-nt -gtr` fixture's bytes with it"""
    from veryfasttree_amd import HipProfileOps, VftError
    from veryfasttree_amd.backend import nj_newick
    ops = HipProfileOps(8, 16, 4, np.float32)
    try:
        z = np.zeros((20, 20), np.float32)
        with pytest.raises(VftError, match="20 states"):
            ops.set_near_posteriors(z, z)
        ops.set_approx_ml(True)
        assert ops.get_approx_ml()
    finally:
        ops.close()
    name = next(n for n in ("full_nt_200_gtr", "full_nt_300_gtr") if os.path.exists(os.path.join(G.GOLDEN, n + ".npz")))
    d = G.load(name)
    run, make, names = G.reference_run(d)
    assert run.n_codes == 4 and run.kwargs.get("gtr")

    def make_on(n, L):
        ops = make(n, L)
        ops.set_approx_ml(True)
        return ops
    assert nj_newick(make_on, d["codes"], names, me_lengths=True, **run.kwargs) == G.text(d["newick"])
