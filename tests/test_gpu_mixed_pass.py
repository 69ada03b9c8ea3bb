"""k_sweep_nt_mixed_multi: four leaf seeds and four profile seeds of a vft_sweep_batch in ONE pass over the targets.

Small states at the edges of the kernel's geometry (VFT_LEAF_SPAN = 1024 leaves per table workgroup, 256 targets per heavy
workgroup, 64 per tile, 16 columns per chunk, VFT_PTILE_M = 112 positions per staged table):

    n = 1300, L = 37    the leaf range is one table span + 276; the leaf / internal boundary sits INSIDE tile 20 (1300 = 20 * 64 + 20)
    n = 1344, L = 130   one span + 320; the boundary is a tile edge but no multiple of 256; L above VFT_PTILE_M

300 sibling pairs joined: 4 full tiles of internal targets and one partly filled.  Gap rate 0.1: explicit-weight and all-gap columns.
Two leaves and two internal nodes are made inactive inside tiles whose other nodes are active.  k = the number of active nodes, so
the hit lists hold the distance, weight and criterion of EVERY active target: equal lists = equal sweeps.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_JOIN = 300
SHAPES = {"n1300_L37": (1300, 37, 11), "n1344_L130": (1344, 130, 12)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)


class _State:
    pass


def _make(shape, dt, option):
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.workload import TopHitsState
    n, L, seed = SHAPES[shape]
    codes = synth.random_descent_codes(n, L, 4, 0.05, 0.1, seed=seed)
    ops = HipProfileOps(n, L, 4, dt)
    assert ops.lib.vft_debug_option(ops.ctx, ctypes.c_int32(12), ctypes.c_int64(option)) == 0
    st = TopHitsState(ops, codes, N_JOIN)
    # inactive nodes in otherwise active tiles: two leaves behind the joined ones, two internal nodes
    off = np.array([2 * N_JOIN + 70, n - 3, n + 5, n + 130])
    parent = st.parent.copy()
    parent[off] = st.maxnode - 1
    ops.set_parents(0, parent)
    s = _State()
    s.ops, s.st, s.n, s.L, s.codes, s.parent = ops, st, n, L, codes, parent
    s.active = np.nonzero(parent < 0)[0]
    s.k = len(s.active)
    return s


@pytest.fixture(scope="module", params=[(sh, dt) for sh in SHAPES for dt in (np.float32, np.float64)],
                ids=lambda p: "%s-%s" % (p[0], np.dtype(p[1]).name))
def trio(request):
    """the same state in three contexts: one launch per seed, per-kind passes only, the built-in choice (mixed pass)"""
    shape, dt = request.param
    t = {opt: _make(shape, dt, opt) for opt in (PER_SEED, NO_MIXED, DEFAULT)}
    yield t
    for s in t.values():
        s.ops.close()


def _seeds(s, n_leaf, n_prof, rng_seed):
    rng = np.random.default_rng(rng_seed)
    leaves = rng.choice(s.active[s.active < s.n], n_leaf, replace=False)
    inner = rng.choice(s.active[s.active >= s.n], n_prof, replace=False)
    seeds = np.concatenate([leaves, inner])
    rng.shuffle(seeds)
    return seeds


def _batch(s, seeds):
    st = s.st
    return s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, s.k)


@pytest.mark.parametrize("n_leaf,n_prof", [(4, 4), (5, 5), (4, 2)])
def test_mixed_pass_equals_per_seed_and_per_kind_passes(trio, n_leaf, n_prof):
    """hits (distance, weight, criterion of every active target), bestJ and the first seed's result arrays: the built-in path - the
    mixed pass for 4 + 4, plus singles for 5 + 5, per-kind groups for 4 + 2 - against one launch per seed and against the per-kind
    passes with the mixed pass switched off."""
    seeds = _seeds(trio[DEFAULT], n_leaf, n_prof, 100 * n_leaf + n_prof)
    got = {}
    for opt, s in trio.items():
        hits, best = _batch(s, seeds)
        got[opt] = (hits, best, s.ops.sweep_results(0, s.st.maxnode))
    for ref in (PER_SEED, NO_MIXED):
        assert np.array_equal(got[DEFAULT][1], got[ref][1])
        assert np.array_equal(got[DEFAULT][0], got[ref][0])
        for a, b in zip(got[DEFAULT][2], got[ref][2]):
            assert np.array_equal(a, b)
    # every active target is in every list, the inactive ones in none
    for h in got[DEFAULT][0]:
        assert np.array_equal(np.sort(h["j"]), trio[DEFAULT].active)


def test_the_mixed_pass_is_what_runs(trio):
    """the kernel-event accounting of a 4 + 4 batch: one launch standing for eight sweeps in single precision (two launches in double
    precision, which keeps the per-kind passes), two with the mixed pass switched off, eight with one launch per seed - so that the
    comparisons above compare what they say they compare."""
    seeds = _seeds(trio[DEFAULT], 4, 4, 3)
    f32 = trio[DEFAULT].ops.dt == np.float32
    for opt, want in ((DEFAULT, 1 if f32 else 2), (NO_MIXED, 2), (PER_SEED, 8)):
        s = trio[opt]
        s.ops.timer_start()
        _batch(s, seeds)
        s.ops.timer_stop_ms()
        assert s.ops.sweep_kernel_ms()[1] == want
        assert s.ops.sweep_kernel_sweeps() == 8


def test_first_slot_results_for_a_leaf_and_a_profile_seed(trio):
    """sweep_results reads slot 0: once a leaf seed, once a profile seed in front of a 4 + 4 batch - the sentinels of the inactive
    targets included."""
    s0 = trio[DEFAULT]
    seeds = _seeds(s0, 4, 4, 7)
    leaf_first = np.concatenate([seeds[seeds < s0.n], seeds[seeds >= s0.n]])
    for order in (leaf_first, leaf_first[::-1].copy()):
        res = {}
        for opt in (PER_SEED, DEFAULT):
            s = trio[opt]
            _batch(s, order)
            res[opt] = s.ops.sweep_results(0, s.st.maxnode)
        for a, b in zip(res[PER_SEED], res[DEFAULT]):
            assert np.array_equal(a, b)
        d, w, c = res[DEFAULT]
        off = s0.parent >= 0
        assert np.all(d[off] == s0.ops.dt.type(1e20)) and np.all(c[off] == s0.ops.dt.type(1e20)) and np.all(w[off] == 0)


def test_mixed_pass_against_the_cpu_oracle(trio):
    """one leaf seed and one profile seed of a 4 + 4 batch against the reference restatement (tests/oracle.py): distance, weight and
    criterion of every active target, bit for bit."""
    from oracle import Oracle
    s = trio[DEFAULT]
    ops, st = s.ops, s.st
    orc = Oracle(ops.dt)
    profs = [ops.profile_download(int(i)) for i in range(st.maxnode)]
    W = np.stack([p[0] for p in profs]); Cc = np.stack([p[1] for p in profs]); F = np.stack([p[2] for p in profs])
    diam, selfw, selfd = ops.get_node_scalars(0, st.maxnode)
    od, na = ops.get_out_distances(0, st.maxnode)
    assert np.all(na[s.active] == st.n_active)   # nothing stale: the oracle's lazy refresh has nothing to do either
    outp, _ = orc.out_profile(W[s.active], Cc[s.active], F[s.active])
    ost = orc.state(s.n, W, Cc, F, s.parent, diam, selfw, selfd, st.totdiam, outp)
    seeds = _seeds(s, 4, 4, 23)
    hits, best = _batch(s, seeds)
    checked = set()
    for slot, q in enumerate(seeds):
        kind = bool(q < s.n)
        if kind in checked:
            continue
        checked.add(kind)
        exp = orc.set_best_hit(ost, int(q), st.n_active, st.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
    assert checked == {True, False}


def _splits(s):
    # tile boundaries inside the leaves (no multiple of 256 or 1024) and inside the internal nodes; the leaf / internal boundary itself
    # where it is a tile boundary (a shard starts at a multiple of 64)
    out = [1088, s.n + 128 - s.n % 64]
    if s.n % 64 == 0:
        out.append(s.n)
    return out


def test_sharded_mixed_pass_merges_to_the_unsharded_lists(trio):
    """set_shard at a tile boundary inside the leaves, inside the internal nodes and at the leaf / internal boundary: the shards'
    top-k merged equal the unsharded top-k.  (A shard without leaves or without internal nodes takes the per-kind passes.)"""
    from veryfasttree_amd.workload import merge_hits
    s = trio[DEFAULT]
    seeds = _seeds(s, 4, 4, 31)
    k = 200
    st = s.st
    whole, best = s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)
    for split in _splits(s):
        parts = []
        for lo, hi in ((0, split), (split, st.maxnode)):
            s.ops.set_shard(lo, hi)
            # (the first batch after set_shard runs seed by seed behind a lazy refresh; the second one takes the shared passes)
            first = s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)[0]
            second = s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)[0]
            assert np.array_equal(first, second)
            parts.append(second)
        s.ops.set_shard(0, st.maxnode)
        for q in range(len(seeds)):
            assert np.array_equal(merge_hits([p[q] for p in parts], k), whole[q]), (split, q)
    again = s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)
    assert np.array_equal(again[0], whole) and np.array_equal(again[1], best)
