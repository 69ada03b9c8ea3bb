"""`-pseudo`, the host half: the arithmetic of correctedPairDistances (host/PseudoDistances.h through vft_pseudo_distances) against a numpy
restatement with the reference's types (NJ.tcc:1460-1488: the sum of dist * weight adds numeric_t products, everything else is double; the
log correction NJ.tcc:322-330 follows), the command line of tools/nj_tree.py, the refusals of the driver, and the fixtures
(tools/gen_pseudo_fixtures.py).  No device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"pseudo_nt_8_ladder": 3, "pseudo_nt_60_frag": 7, "pseudo_nt_200_frag": 3, "pseudo_aa_80_frag": 2}   # name: runs


def log_correct(d, scoredist):
    """NJ.tcc:322-330 with libm's log on a double"""
    if not scoredist:
        d = -0.75 * math.log(1.0 - d * 4.0 / 3.0) if d < 0.74 else 3.0
    else:
        d = -1.3 * math.log(1.0 - d) if d < 0.99 else 3.0
    return d if d < 3.0 else 3.0


def restated(dist, weight, pseudo, scoredist, float_product=True):
    """NJ.tcc:1471-1483 with the types of a run whose numeric_t is dist.dtype; float_product=False: the sum's products formed in double
    instead (what the reference does NOT do) - for the case that tells the two apart"""
    dt = dist.dtype.type
    top, bottom = 0.0, 0.0
    for d, w in zip(dist, weight):
        top += float(dt(d) * dt(w)) if float_product else float(d) * float(w)
        bottom += float(w)
    prior = top / bottom if bottom > 0.01 else 3.0
    out = [(float(d) * float(w) + prior * pseudo) / (float(w) + pseudo) for d, w in zip(dist, weight)]
    return np.array([log_correct(x, scoredist) for x in out]), prior


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("scoredist", [False, True])
@pytest.mark.parametrize("n", [3, 6])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_random_pairs(dt, n, scoredist):
    from veryfasttree_amd.backend import pseudo_distances
    rng = np.random.default_rng(7 + n)
    for trial in range(200):
        dist = rng.uniform(0.0, 1.1, n).astype(dt)          # beyond 0.74 / 0.99: the capped branch of the log correction too
        weight = (rng.uniform(0.0, 120.0, n) * (rng.random(n) < 0.85)).astype(dt)
        for pseudo in (1.0, 0.5, 3.0):
            want, _ = restated(dist, weight, pseudo, scoredist)
            assert same_bits(pseudo_distances(dist, weight, pseudo, scoredist), want), (trial, pseudo, dist, weight)
        # weight 0 = off: the log-corrected distances alone
        assert same_bits(pseudo_distances(dist, weight, 0.0, scoredist), [log_correct(float(d), scoredist) for d in dist])


@pytest.mark.parametrize("n", [3, 6])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_all_weights_zero_take_the_prior_of_three(dt, n):
    from veryfasttree_amd.backend import pseudo_distances
    dist = np.linspace(0.1, 1.0, n).astype(dt)     # (profileDist answers 1.0 for a pair without a common column; any value must do)
    for scoredist in (False, True):
        got = pseudo_distances(dist, np.zeros(n, dt), 1.0, scoredist)
        assert same_bits(got, np.full(n, 3.0))       # (0 * d + 3 * 1) / (0 + 1) = 3, and logCorrect caps at 3


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_prior_switches_at_a_total_weight_of_one_hundredth(dt):
    from veryfasttree_amd.backend import pseudo_distances
    dist = np.array([0.2, 0.3, 0.1, 0.25, 0.15, 0.05], dt)
    for total, branch in ((0.0099, "three"), (0.0101, "mean")):
        weight = np.full(6, total / 6, dt)
        bottom = sum(float(w) for w in weight)
        assert (bottom > 0.01) == (branch == "mean")
        want, prior = restated(dist, weight, 1.0, False)
        assert (prior == 3.0) == (branch == "three")
        assert same_bits(pseudo_distances(dist, weight, 1.0, False), want)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_pair_of_weight_zero_gets_exactly_the_prior(dt):
    from veryfasttree_amd.backend import pseudo_distances
    dist = np.array([0.21, 0.33, 1.0, 0.12, 0.27, 0.18], dt)
    weight = np.array([40, 33, 0, 51, 12, 8], dt)
    want, prior = restated(dist, weight, 1.0, False)
    got = pseudo_distances(dist, weight, 1.0, False)
    assert same_bits(got, want)
    assert 0 < prior < 0.74 and got[2] == log_correct(prior, False)      # (0 * 1.0 + prior * 1) / (0 + 1)


def test_the_sum_adds_float_products():
    """a float run: dTop adds dist * weight as a FLOAT product.  A quartet for which the double product gives other bits is found by search
    (most do: the product of two floats rarely fits 24 bits), and the library must agree with the float restatement, not the double one"""
    from veryfasttree_amd.backend import pseudo_distances
    rng = np.random.default_rng(99)
    found = 0
    for trial in range(2000):
        dist = rng.uniform(0.01, 0.7, 6).astype(np.float32)
        weight = rng.uniform(1.0, 200.0, 6).astype(np.float32)
        as_float, _ = restated(dist, weight, 1.0, False, True)
        as_double, _ = restated(dist, weight, 1.0, False, False)
        if same_bits(as_float, as_double):
            continue
        found += 1
        got = pseudo_distances(dist, weight, 1.0, False)
        assert same_bits(got, as_float) and not same_bits(got, as_double), (dist, weight)
        if found == 50:
            break
    assert found == 50


def test_bad_arguments():
    from veryfasttree_amd.backend import pseudo_distances, VftError
    d = np.full(6, 0.2, np.float32)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(VftError):
            pseudo_distances(d, d, bad)
    with pytest.raises(VftError):
        pseudo_distances(d[:4], d[:4], 1.0)


def load_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nj_tree
    return nj_tree


def test_the_tool_parses_the_option():
    t = load_tool()
    run_of = lambda args: t.translate(args)[1]
    assert "pseudo" not in run_of(["in.fa", "-full"]).kwargs
    assert run_of(["in.fa", "-full", "-pseudo"]).kwargs["pseudo"] == 1.0                                  # last
    run = run_of(["in.fa", "-pseudo", "-nosupport"])                                                     # before another flag
    assert run.kwargs["pseudo"] == 1.0 and run.n_bootstrap == 0
    run = run_of(["in.fa", "-pseudo", "0.5", "-full"])
    assert run.kwargs["pseudo"] == 0.5 and run.kwargs["ml_nni"] == 20
    assert run_of(["in.fa", "-pseudo", "3"]).kwargs["pseudo"] == 3.0
    assert run_of(["in.fa", "-pseudo", "0"]).kwargs["pseudo"] == 0.0
    for bad in ("-1", "-0.5", "nan", "inf"):
        with pytest.raises(SystemExit) as e:
            t.translate(["in.fa", "-pseudo", bad])
        assert "-pseudo" in str(e.value)


class NoDevice:
    """stands where a context would: the refusals below come before anything looks at it"""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)


def newick_without_a_device(**kw):
    from veryfasttree_amd import backend
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    return backend.nj_newick(lambda n, L: NoDevice(), codes, ["s%d" % k for k in range(6)], me_lengths=True, **kw)


def test_the_driver_refuses_a_bad_weight_before_the_device():
    from veryfasttree_amd.backend import VftError
    for bad in (-1.0, -1e-300, float("nan"), float("inf")):
        with pytest.raises(VftError, match="-pseudo takes a finite weight >= 0"):
            newick_without_a_device(pseudo=bad)


def test_the_driver_refuses_several_ranks_before_the_device():
    from veryfasttree_amd import backend

    class TwoRanks:   # (never called: the refusal comes first)
        struct = backend._Comm(0, 2, backend._ALLGATHER(lambda user, nbytes, device: 1), None, None, None, 0, None, None, 0)

        def pointer(self):
            return C.cast(C.pointer(self.struct), C.c_void_p)

    with pytest.raises(backend.VftError, match="-pseudo with a vft_comm of more than one rank"):
        newick_without_a_device(pseudo=1.0, comm=TwoRanks())


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_load_and_differ_from_their_controls(name):
    d = G.load(name)
    assert int(d["n_runs"]) == FIXTURES[name]
    for k in range(FIXTURES[name]):
        pre = "r%d_" % k
        flags = bytes(d[pre + "flags"]).decode().split()
        assert "-pseudo" in flags and float(d[pre + "pseudo"]) > 0
        for key in ("newick", "newick_support"):
            got, ctl = bytes(d[pre + key]), bytes(d[pre + "control_" + key])
            assert got.strip().endswith(b";") and ctl.strip().endswith(b";")
            assert got != ctl or (key == "newick_support" and "-nosupport" in flags), (name, k, key)
        assert bytes(d[pre + "newick"]) != bytes(d[pre + "control_newick"])
        if "-noml" not in flags:
            assert len(d[pre + "loglk"]) >= 1 and len(d[pre + "rates"]) == 20 and len(d[pre + "ratecat"]) == d["codes"].shape[1]
