"""`-pseudo` on the device and end to end.

The walk server answers the pairs' weights next to their distances (vft_walk_submit_w / _collect_w / _step_w: bit 22 of the command,
csrc/vft_kernels_walk.h): one context is driven through the server, an identical second one through the plain calls
(vft_average_chain + vft_profile_distances), and all six distances and all six weights of every step must carry the same bits - with
flagged and flagless steps interleaved in one session, both placements of the mailbox and both strides.

Whole runs of the reference with `-pseudo [W]` (tools/gen_pseudo_fixtures.py) against nj_newick(..., pseudo=W), byte for byte, and the
same flags without the option against pseudo=0."""
import ctypes as C

import numpy as np
import pytest

import golden_util as G
from test_gpu_chains import ptr, same
from test_gpu_walk_server import I32, I64, U32, OPT_DEVICE_MAIL, OPT_NO_SERVER, OPT_STRIDE, init_scratch, random_steps

pytestmark = pytest.mark.gpu

ERR_INVALID = 1
RUNS = [("pseudo_nt_8_ladder", k) for k in range(3)] + [("pseudo_nt_60_frag", k) for k in range(7)] + \
       [("pseudo_nt_200_frag", k) for k in range(3)] + [("pseudo_aa_80_frag", k) for k in range(2)]


# ------------------------------------------------------------------------------------------------ the walk server's weights
def make_fragment_state(dt, n_codes, L, seed):
    """test_gpu_chains.make_state with fragments among the leaves: leaves 0 and 2 hold the first half of the columns only, leaves 1 and 3
    the second half only - a pair across the halves has no common column.  48 leaves, 47 internal rows, ids 95.. free."""
    from veryfasttree_amd import HipProfileOps, synth
    n = 48
    rng = np.random.default_rng(seed)
    codes = synth.random_descent_codes(n, L, n_codes, 0.15, 0.05, seed=seed)
    codes[[0, 2], L // 2:] = synth.NOCODE
    codes[[1, 3], :L // 2] = synth.NOCODE
    ops = HipProfileOps(n, L, n_codes, dt, max_nodes=8 * n)
    if n_codes == 20:
        from veryfasttree_amd.backend import distance_tables
        t = distance_tables(None, dt)
        ops.set_distance_matrix(t["distances"], t["codefreq"], t["eigenval"], t["eigentot"])
    ops.upload_leaves(codes)
    for v in range(n, 2 * n - 1):
        a, b = rng.choice(np.arange(4, v), 2, replace=False)   # (the internal rows keep off the four fragments)
        ops.averageProfile([v], [int(a)], [int(b)])
    ops.set_max_node(8 * n)
    assert ops.lib.vft_set_profile_rows(ops.ctx, I32(1)) == 0
    return ops, rng, 2 * n - 1


def plain_step_w(ops, dt, out, a, b, q):
    if len(out):
        assert ops.lib.vft_average_chain(ops.ctx, I32(len(out)), ptr(out), ptr(a), ptr(b)) == 0
    pi = np.array([q[0], q[0], q[0], q[1], q[1], q[2]], np.int64)
    pj = np.array([q[1], q[2], q[3], q[2], q[3], q[3]], np.int64)
    d, w = ops.profileDist(pi, pj)
    return np.asarray(d, dt), np.asarray(w, dt)


def disjoint_step(rng, free):
    """a step whose quartet holds pairs without a common column: A = average(leaf 0, leaf 2), a row of the first half written by this very
    step; B, C = leaves 1 and 3 (second half), D = leaf 0 (first half): AB, AC, BD and CD have no common column, AD and BC have"""
    x = free + int(rng.integers(0, 24))
    out, a, b = np.array([x], np.int64), np.array([0], np.int64), np.array([2], np.int64)
    return out, a, b, np.array([x, 1, 3, 0], np.int64)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("dt,nc,L,stride,device_mail", [
    (np.float32, 4, 137, 8, 0), (np.float32, 4, 137, 1, 1), (np.float32, 4, 137, 8, 1), (np.float32, 4, 137, 1, 0),
    (np.float64, 4, 200, 8, 0), (np.float64, 4, 200, 1, 1),
    (np.float32, 20, 90, 8, 0), (np.float32, 20, 90, 1, 1),
    (np.float64, 20, 300, 8, 0), (np.float64, 20, 300, 1, 1)])
def test_server_weights_equal_the_plain_calls(dt, nc, L, stride, device_mail):
    s_ops, rng, free = make_fragment_state(dt, nc, L, seed=21)
    p_ops, _, _ = make_fragment_state(dt, nc, L, seed=21)
    init_scratch([s_ops, p_ops], free)
    steps = random_steps(rng, free, 60, long_every=11)
    for t in range(2, len(steps), 5):           # a fifth of the steps: pairs without a common column
        steps[t] = disjoint_step(rng, free)
    lib, ctx = s_ops.lib, s_ops.ctx
    err = lambda: lib.vft_last_error(ctx)
    assert lib.vft_debug_option(ctx, I32(OPT_STRIDE), I64(stride)) == 0
    assert lib.vft_debug_option(ctx, I32(OPT_DEVICE_MAIL), I64(device_mail)) == 0
    assert lib.vft_walk_server_start(ctx) == 0, err()

    def check(t, d1, w1):
        out, a, b, q = steps[t]
        d2, w2 = plain_step_w(p_ops, dt, out, a, b, q)
        assert np.array_equal(bits(d1), bits(d2)), (t, d1, d2)
        if w1 is not None:
            assert np.array_equal(bits(w1), bits(w2)), (t, w1, w2)
        if t % 5 == 2:
            # AB, AC have no common column: profileDist's denominator is 0, and Besthit::weight is then the reference's stand-in
            # (dist, weight) = (1, 0.01) (NJ.tcc:1187-1188) - what the plain call returns and the server must return too; BC has columns
            # BD, CD are pairs of LEAVES: the device answers seqDist for those (NJ.tcc:1601-1623), whose weight is the number of common
            # columns - exactly 0.  AD and BC have columns.
            assert d2[0] == 1 and d2[1] == 1 and w2[0] == dt(0.01) and w2[1] == dt(0.01) and w2[2] > 0 and w2[3] >= 1, (t, d2, w2)
            assert d2[4] == 1 and d2[5] == 1 and w2[4] == 0 and w2[5] == 0, (t, d2, w2)
            assert w1 is None or (w1[0] == dt(0.01) and w1[1] == dt(0.01) and w1[4] == 0 and w1[5] == 0)

    empty = 0
    t = 0
    while t < len(steps):
        out, a, b, q = steps[t]
        kind = t % 4
        if kind == 0 or t + 1 >= len(steps):    # one flagged step
            d1, w1 = np.full(6, -1, dt), np.full(6, -1, dt)
            assert lib.vft_walk_step_w(ctx, I32(len(out)), ptr(out), ptr(a), ptr(b), ptr(q), ptr(d1), ptr(w1)) == 0, err()
            check(t, d1, w1)
            empty += int((w1 == dt(0.01)).sum())
            t += 1
        elif kind == 1:                         # a flagless step between them: answered as ever
            d1 = np.full(6, -1, dt)
            assert lib.vft_walk_step(ctx, I32(len(out)), ptr(out), ptr(a), ptr(b), ptr(q), ptr(d1)) == 0, err()
            check(t, d1, None)
            t += 1
        else:                                   # two tickets in flight, the first with the flag, the second alternating
            flagged = [True, (t // 4) % 2 == 0]
            tickets = []
            for k in range(2):
                o2, a2, b2, q2 = steps[t + k]
                tk = U32(0)
                submit = lib.vft_walk_submit_w if flagged[k] else lib.vft_walk_submit
                assert submit(ctx, I32(len(o2)), ptr(o2), ptr(a2), ptr(b2), ptr(q2), C.byref(tk)) == 0, err()
                tickets.append(tk)
            for k in range(2):
                d1, w1 = np.full(6, -1, dt), np.full(6, -1, dt)
                if flagged[k]:
                    # the wrong collect is refused as a bad argument, waits for nothing and leaves the ticket (and the server) as they were
                    assert lib.vft_walk_collect(ctx, tickets[k], ptr(d1)) == ERR_INVALID
                    assert lib.vft_walk_collect_w(ctx, tickets[k], ptr(d1), ptr(w1)) == 0, err()
                    check(t + k, d1, w1)
                    empty += int((w1 == dt(0.01)).sum())
                else:
                    assert lib.vft_walk_collect_w(ctx, tickets[k], ptr(d1), ptr(w1)) == ERR_INVALID
                    assert lib.vft_walk_collect(ctx, tickets[k], ptr(d1)) == 0, err()
                    check(t + k, d1, None)
            t += 2
    assert empty >= 8                           # the weights of empty pairs did come back through the server
    assert lib.vft_walk_server_stop(ctx) == 0, err()
    for x in range(48, free + 24):
        assert same(s_ops.profile_download(x), p_ops.profile_download(x)), x
    s_ops.close()
    p_ops.close()


def test_step_w_without_a_server_is_a_state_error():
    s_ops, _, free = make_fragment_state(np.float32, 4, 137, seed=5)
    assert s_ops.lib.vft_debug_option(s_ops.ctx, I32(OPT_NO_SERVER), I64(1)) == 0
    assert s_ops.lib.vft_walk_server_start(s_ops.ctx) == 3
    q = np.array([0, 1, 2, 3], np.int64)
    out = np.zeros(0, np.int64)
    d, w = np.zeros(6, np.float32), np.zeros(6, np.float32)
    assert s_ops.lib.vft_walk_step_w(s_ops.ctx, I32(0), ptr(out), ptr(out), ptr(out), ptr(q), ptr(d), ptr(w)) == 3   # the caller makes the two plain calls
    s_ops.close()


# ------------------------------------------------------------------------------------------------ whole trees
def case(name, k, control):
    """run k of a fixture (or its control: the same flags without -pseudo) as the arguments of nj_newick"""
    d = G.load(name)
    pre = "r%d_" % k
    run, make, names = G.reference_run(d, pre)
    assert run.kwargs["pseudo"] == float(d[pre + "pseudo"])
    kw = dict(run.kwargs, pseudo=0.0) if control else run.kwargs
    want = {key: d[pre + ("control_" if control else "") + key] for key in ("newick", "newick_support", "loglk", "rates", "ratecat")
            if pre + ("control_" if control else "") + key in d}
    return d, G.text(d[pre + "flags"]).split(), make, names, kw, run.n_bootstrap, want


text = G.text


@pytest.mark.parametrize("control", [False, True], ids=["pseudo", "control"])
@pytest.mark.parametrize("name,k", RUNS)
def test_trees_match_the_reference(name, k, control):
    """the run's flags, with and without supports, byte for byte; the ML runs add the TreeLogLk lines, the rates and the site categories
    as the ml_* / intree tests compare them.  control: the same flags without -pseudo through the same code with pseudo=0."""
    d, flags, make, names, kw, n_boot, want = case(name, k, control)
    G.assert_trees_match_the_reference("%s %d" % (name, k), make, d["codes"], names, kw, want, n_bootstrap=n_boot)


def test_one_tree_three_routes():
    """pseudo_nt_60_frag's `-noml -pseudo`: through the walk server, with a launch per step (the plain calls return the weights), and on
    the lockstep lanes of `-threads 4` (against that run's own fixture) - all three reach the reference"""
    from veryfasttree_amd.backend import nj_newick, DEBUG_NO_WALK_SERVER
    d, flags, make, names, kw, _, want = case("pseudo_nt_60_frag", 0, False)
    assert flags == ["-nt", "-noml", "-pseudo"] and kw["threads"] == 1
    ref = text(want["newick_support"])
    assert nj_newick(make, d["codes"], names, me_lengths=True, n_bootstrap=1000, **kw) == ref
    assert nj_newick(make, d["codes"], names, me_lengths=True, n_bootstrap=1000, debug_flags=DEBUG_NO_WALK_SERVER, **kw) == ref
    d4, flags4, make4, names4, kw4, _, want4 = case("pseudo_nt_60_frag", 6, False)
    assert flags4 == flags and kw4["threads"] == 4
    assert nj_newick(make4, d4["codes"], names4, me_lengths=True, n_bootstrap=1000, **kw4) == text(want4["newick_support"])


def test_no_dual_commands_with_pseudocounts():
    """the comparison of a dual command works on distances without pseudocounts: none is sent while pseudo > 0 (the SPR chains wait for the
    host's verdict, as with VFT_NJ_DEBUG_NO_WALK_DUAL); the control on the same alignment sends them"""
    from veryfasttree_amd.backend import nj_newick, last_walk_dual
    d, flags, make, names, kw, _, want = case("pseudo_nt_200_frag", 0, False)
    kw = dict(kw, ml_nni=0)   # (the minimum-evolution stages are where the chains run)
    assert kw["me_nni"] and kw["spr"] == 2
    nj_newick(make, d["codes"], names, me_lengths=True, **kw)
    assert last_walk_dual() == (0, 0)
    nj_newick(make, d["codes"], names, me_lengths=True, **dict(kw, pseudo=0.0))
    sent, taken = last_walk_dual()
    assert sent > 0 and taken > 0
