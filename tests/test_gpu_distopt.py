"""`-rawdist` for a tree and `-trans FILE` on the device and end to end.

Whole runs of the reference (tools/gen_distopt_fixtures.py) through refflags.from_reference_flags and nj_newick, byte for byte, each followed
in the same process by its control - the same flags without the option - which must still print the control's tree: neither switch may
leak.  WAG's own constants as a `-trans` file print the tree of an existing `-wag` fixture.  `-rawdist` with SPR rounds sends dual
commands to the walk server and takes them (the comparison of six uncorrected distances on the device, bit 23 of the command), and prints
the same tree without them.  vft_split_supports with the switch on against a numpy restatement of splitSupport (NJ.tcc:607-702) without
its logCorrect, in the one-pass kernel and - at 1 707 columns - the pass kernel.  tools/nj_tree.py with each option."""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA = "ARNDCQEGHILKMFPSTWYV"
RUNS = [("rawdist_nt_60", k) for k in range(10)] + [("rawdist_aa_40", k) for k in range(4)] + [("rawdist_nt_16x1707", 0)] + \
       [("trans_aa_40", k) for k in range(6)] + [("trans_aa_12x2200", 0)]
_fixtures = {}


def fixture(name):
    if name not in _fixtures:
        _fixtures[name] = G.load(name)
    return _fixtures[name]


def reference_call(d, pre, control=False):
    """(make_ops, names, the keywords of nj_newick, the resamples) of run `pre` of fixture d - of its control: the same flags, the option
    taken out.  What refflags leaves in `other` is acted on here: rawdist -> nj_newick(rawdist=True), trans -> aa_trans = the file's text."""
    flags = G.text(d[pre + "flags"]).split()
    if control:
        k = flags.index("-trans") if "-trans" in flags else flags.index("-rawdist")
        flags = flags[:k] + flags[k + (2 if flags[k] == "-trans" else 1):]
    run, make, names = G.reference_run(dict(d, **{pre + "flags": np.frombuffer(" ".join(flags).encode(), np.uint8)}), pre)
    kw = dict(run.kwargs)
    assert set(run.other) <= {"rawdist", "trans"} and bool(run.other) != control
    if "rawdist" in run.other:
        kw["rawdist"] = True
    if "trans" in run.other:
        kw["aa_trans"] = bytes(d["trans_text"])
    return make, names, kw, run.n_bootstrap


def wanted(d, pre):
    return {key[len(pre):]: d[key] for key in d if key.startswith(pre) and key[len(pre):] in ("newick", "newick_support", "loglk", "rates", "ratecat")}


def assert_run_matches(label, make, codes, names, kw, want, n_boot):
    """golden_util.assert_trees_match_the_reference; a `-nocat` run has one rate where that helper expects the 20 of the CAT approximation:
    the same comparisons of the likelihoods and the trees, and the one rate"""
    from veryfasttree_amd.backend import nj_newick
    if kw.get("ml_nni") != 1 and kw.get("mllen") != 1:
        return G.assert_trees_match_the_reference(label, make, codes, names, kw, want, n_boot)
    tree, loglk, rates, ratecat = nj_newick(make, codes, names, me_lengths=True, return_rates=True, **kw)
    print(label, "TreeLogLk", list(loglk), "reference", list(want["loglk"]))
    assert len(loglk) == len(want["loglk"])
    assert np.allclose(loglk, want["loglk"], rtol=2e-6 if kw["dtype"] == np.float32 else 1e-8, atol=6e-5), (loglk, want["loglk"])
    assert list(rates) == [1.0] == list(want["rates"]) and not ratecat.any() and not want["ratecat"].any()
    assert tree == G.text(want["newick"])
    assert nj_newick(make, codes, names, me_lengths=True, n_bootstrap=n_boot, **kw) == G.text(want["newick_support"])


@pytest.mark.parametrize("name,k", RUNS, ids=["%s-r%d" % r for r in RUNS])
def test_every_run_prints_the_references_tree_and_its_control_after_it(name, k):
    d = fixture(name)
    pre = "r%d_" % k
    make, names, kw, n_boot = reference_call(d, pre)
    assert_run_matches(name + " " + G.text(d[pre + "flags"]), make, d["codes"], names, kw, wanted(d, pre), n_boot)
    # the control, in the same process and behind the run with the option: nothing of it is left
    make, names, kw, n_boot = reference_call(d, pre, control=True)
    assert "rawdist" not in kw and "aa_trans" not in kw
    assert_run_matches(name + " control", make, d["codes"], names, kw, wanted(d, pre + "control_"), n_boot)


def model_text(matrix, stat, fmt):
    lines = ["\t".join(AA) + "\t*"]
    for i in range(20):
        lines.append("\t".join([AA[i]] + [fmt % matrix[i, j] for j in range(20)] + [fmt % stat[i]]))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("beside", ["jtt", "wag", "lg"])
def test_wags_own_matrix_as_a_file_prints_the_wag_tree(beside):
    """`-wag -double-precision` of an existing fixture; the model named beside the file does not matter (the file wins)"""
    from veryfasttree_amd.backend import aa_model_matrix, nj_newick
    d = G.load("full_aa_90_wag_double")
    run, make, names = G.reference_run(d)
    assert run.kwargs["aa_model"] == "wag"
    kw = dict(run.kwargs, aa_model=beside, aa_trans=model_text(*aa_model_matrix("wag"), fmt="%.17g"))
    tree, loglk = nj_newick(make, d["codes"], names, me_lengths=True, return_loglk=True, **kw)
    assert np.allclose(loglk, d["loglk"], rtol=1e-8, atol=6e-5)
    assert tree == G.text(d["newick"])


def test_rawdist_spr_chains_compare_on_the_device():
    """`-nt -noml -rawdist` on 60 x 80: two SPR rounds whose chains hand both continuations to the walk server; the host checks every
    choice the workgroups made against its own comparison of the same six uncorrected distances (MLLengths::sprAttempt throws otherwise)"""
    from veryfasttree_amd.backend import DEBUG_NO_WALK_DUAL, last_walk_dual, nj_newick
    d = fixture("rawdist_nt_60")
    assert G.text(d["r1_flags"]) == "-nt -noml -rawdist"
    make, names, kw, _ = reference_call(d, "r1_")
    assert kw["spr"] == 2 and kw["rawdist"] is True
    kept = []

    def make_kept(n, L):
        kept.append(make(n, L))
        return kept[-1]
    tree = nj_newick(make_kept, d["codes"], names, me_lengths=True, **kw)
    sent, taken = last_walk_dual()
    print("dual commands sent", sent, "taken", taken)
    assert kept[0].get_raw_distances() is True
    assert sent > 0 and 0 < taken <= sent
    assert tree == G.text(d["r1_newick"])
    assert nj_newick(make, d["codes"], names, me_lengths=True, debug_flags=DEBUG_NO_WALK_DUAL, **kw) == tree
    assert last_walk_dual() == (0, 0)
    # and the control: the log-corrected comparison, dual commands as ever
    make, names, kw, _ = reference_call(d, "r1_", control=True)
    assert nj_newick(make, d["codes"], names, me_lengths=True, **kw) == G.text(d["r1_control_newick"])
    assert last_walk_dual()[1] > 0


# ------------------------------------------------------------------------------------------------ the supports, called directly
def restated_supports(profiles, quartets, col, correct):
    """splitSupport (NJ.tcc:607-702): per pair and column the weight (a numeric_t product) and the weighted profileDistPiece (double; no
    distance matrix), per resample their sums in double, in column order; dist = totw > 0.01 ? totp / totw : 3; `correct` = logCorrect
    or nothing; supported when AC + BD and AD + BC both exceed AB + CD"""
    f32 = np.float32

    def pieces(p1, p2):
        (w1, c1, f1), (w2, c2, f2) = p1, p2
        w = (w1 * w2).astype(f32).astype(np.float64)          # a numeric_t product, widened (NJ.tcc:624-629)
        dist = np.zeros(len(w))                               # profileDistPiece without a matrix (NJ.tcc:918-939), in double
        both = (c1 != 127) & (c2 != 127)
        dist[both] = (c1[both] != c2[both]).astype(np.float64)
        one = (c1 != 127) & (c2 == 127)
        dist[one] = 1.0 - f2[one, c1[one]].astype(np.float64)
        two = (c1 == 127) & (c2 != 127)
        dist[two] = 1.0 - f1[two, c2[two]].astype(np.float64)
        none = (c1 == 127) & (c2 == 127)
        piece = np.ones(len(w))
        for k in range(4):
            piece -= (f1[:, k] * f2[:, k]).astype(f32).astype(np.float64)   # piece -= f1[k] * f2[k]: a numeric_t product
        dist[none] = piece[none]
        return np.where(w > 0, w * dist, 0.0), w

    out = np.zeros(len(quartets))
    for t, q in enumerate(quartets):
        dist = []
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            piece, w = pieces(profiles[q[i]], profiles[q[j]])
            totp, totw = np.cumsum(piece[col], axis=1)[:, -1], np.cumsum(w[col], axis=1)[:, -1]      # (cumsum adds in order, as the loop does)
            dist.append(np.array([correct(p / ww if ww > 0.01 else 3.0) for p, ww in zip(totp, totw)]))
        out[t] = (((dist[1] + dist[4] - dist[0] - dist[5]) > 0) & ((dist[2] + dist[3] - dist[0] - dist[5]) > 0)).sum() / col.shape[0]
    return out


def jukes_cantor(x):
    return min(3.0, -0.75 * np.log(1.0 - x * 4.0 / 3.0) if x < 0.74 else 3.0)


@pytest.mark.parametrize("n_pos,seed", [(150, 5), (1707, 93)], ids=["one-pass-kernel", "pass-kernel-1707"])
def test_split_supports_without_the_correction(n_pos, seed):
    """16 leaves and 10 averaged rows; quartets of leaves, of rows, and mixed; 1 and 100 resamples.  Switch on: the restatement without
    logCorrect; off again: the restatement with it - and the two differ somewhere, so the switch is what decides"""
    from veryfasttree_amd import HipProfileOps, synth
    from test_gpu_long_supports import knuth_columns
    n = 16
    codes = synth.random_descent_codes(n, n_pos, 4, 0.25, 0.03, seed)
    ops = HipProfileOps(n, n_pos, 4, np.float32, max_nodes=4 * n)
    ops.upload_leaves(codes)
    rng = np.random.default_rng(seed)
    for v in range(n, n + 10):
        a, b = rng.choice(np.arange(v), 2, replace=False)
        ops.averageProfile([v], [int(a)], [int(b)])
    ops.set_max_node(n + 10)
    profiles = {v: ops.profile_download(v) for v in range(n + 10)}
    quartets = [(0, 1, 2, 3), (4, 9, 13, 7), (16, 17, 18, 19), (20, 5, 21, 11), (25, 24, 23, 22), (3, 12, 24, 18), (8, 10, 14, 15), (19, 2, 6, 25)]
    a, b, c, dd = (np.array(x, np.int64) for x in zip(*quartets))
    differ = 0
    for n_boot in (1, 100):
        col = knuth_columns(n_boot, n_pos)
        assert ops.get_raw_distances() is False
        corrected = ops.split_supports(a, b, c, dd, col)
        ops.set_raw_distances(True)
        assert ops.get_raw_distances() is True
        raw = ops.split_supports(a, b, c, dd, col)
        ops.set_raw_distances(False)
        assert np.array_equal(ops.split_supports(a, b, c, dd, col), corrected)
        want_raw = restated_supports(profiles, quartets, col, lambda x: x)
        print(n_pos, n_boot, "raw", raw, "corrected", corrected)
        assert np.array_equal(raw, want_raw), (raw, want_raw)
        if n_pos < 1000:      # (the corrected flavour is every other supports test's business: once here, on the short case)
            assert np.array_equal(corrected, restated_supports(profiles, quartets, col, jukes_cantor))
        differ += int((raw != corrected).sum())
    assert differ > 0


# ------------------------------------------------------------------------------------------------ the tool
def run_tool(tmp_path, d, alphabet, args):
    from veryfasttree_amd import synth
    fa = str(tmp_path / "in.fa")
    synth.codes_to_fasta(d["codes"], fa, alphabet)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    return res.stdout.decode().strip()


def test_tool_rawdist(tmp_path):
    from veryfasttree_amd import synth
    d = fixture("rawdist_nt_60")
    assert G.text(d["r1_flags"]) == "-nt -noml -rawdist"
    assert run_tool(tmp_path, d, synth.ALPHABET_NT, ["-full", "-noml", "-rawdist"]) == G.text(d["r1_newick_support"])


def test_tool_trans(tmp_path):
    from veryfasttree_amd import synth
    d = fixture("trans_aa_40")
    assert G.text(d["r1_flags"]) == "-nome -mllen -trans model.txt"
    model = tmp_path / "model.txt"
    model.write_bytes(bytes(d["trans_text"]))
    assert run_tool(tmp_path, d, synth.ALPHABET_AA, ["-aa", "-mllen", "-trans", str(model)]) == G.text(d["r1_newick_support"])
    bad = tmp_path / "bad.txt"
    bad.write_bytes(bytes(d["trans_text"]).replace(b"\t*", b"", 1))
    fa = str(tmp_path / "in.fa")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-aa", "-mllen", "-trans", str(bad)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert res.returncode != 0 and "Invalid header line in transition matrix file" in res.stderr.decode()
