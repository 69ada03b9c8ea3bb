"""k_sweep_nt_mixed_multi's leaf targets: ONE walk over a span's compacted leaves for the four profile seeds (addend tables in LDS) and
the four leaf seeds (popcounts on the chunk the walk already holds) - vft_leaf_table_wg_mixed.

The same state in three contexts with vft_debug_option 12 = 1 (one launch per seed), 8 (per-kind passes) and 0 (the built-in choice:
the mixed pass in single precision).  k = the number of active nodes, so the hit lists hold the distance, weight and criterion of
EVERY active target: equal lists = equal sweeps.

Shapes at the walk's edges (VFT_LEAF_SPAN = 1024 leaves per span, two rounds of 2 x 256 leaves, 16 columns per chunk, VFT_PTILE_M =
112 columns = 7 chunks per staged table):

    n = 1300, L = 37     one span + 276 ids; the leaf / internal boundary inside a tile
    n = 2600, L = 113    a second table tile for a single column; a third span of 552 ids
    n = 1344, L = 230    three table tiles, the last chunk partly padding

Active leaves per span (set_parents; random positions, so inactive leaves sit inside otherwise active tiles): 0, 1, 255, 256, 257, 512,
513 and all 1024 - one leaf per lane or two (NBT = 1 / 2), one round of the span or two.

Leaf seeds: ids n - 10 .. n - 4 are always active; four of them have a gap in column 0, in the last column of a chunk (15), in the
first of the next (16) and in the last real column (L - 1), two more hold the same sequence.  Every leaf seed is an active leaf and
therefore a target of its own span.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_JOIN = 300
NOCODE = 127
SPAN = 1024
SHAPES = {"n1300_L37": (1300, 37, 21), "n2600_L113": (2600, 113, 22), "n1344_L230": (1344, 230, 23)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)
# active leaves per span; the last span also keeps its special leaves (so at least 7 there)
PATTERNS = {
    "n1300_L37": [(1024, 276), (0, 8), (1, 100), (513, 256), (255, 257)],
    "n2600_L113": [(0, 1, 552), (255, 256, 300), (257, 512, 8), (513, 1024, 257), (1024, 0, 512)],
    "n1344_L230": [(256, 257), (1024, 320), (512, 9), (1, 255)],
}


class _State:
    pass


def _special(n):
    """gap0, gap15, gap16, gapLast, twinA, twinB, plain: leaves that every pattern keeps active"""
    return np.arange(n - 10, n - 3)


def _codes(shape):
    from veryfasttree_amd import synth
    n, L, seed = SHAPES[shape]
    codes = synth.random_descent_codes(n, L, 4, 0.05, 0.1, seed=seed)
    g0, g15, g16, gl, ta, tb, _ = _special(n)
    codes[g0, 0] = NOCODE
    codes[g15, 15] = NOCODE
    codes[g16, 16] = NOCODE
    codes[gl, L - 1] = NOCODE
    codes[tb] = codes[ta]
    return codes


def _make(shape, dt, option):
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.workload import TopHitsState
    n, L, _ = SHAPES[shape]
    codes = _codes(shape)
    ops = HipProfileOps(n, L, 4, dt)
    assert ops.lib.vft_debug_option(ops.ctx, ctypes.c_int32(12), ctypes.c_int64(option)) == 0
    st = TopHitsState(ops, codes, N_JOIN)
    s = _State()
    s.ops, s.st, s.n, s.L, s.codes, s.shape = ops, st, n, L, codes, shape
    _set_parent(s, _base_parent(s))
    return s


def _base_parent(s):
    """the state as joined (leaves 0 .. 599 inactive), plus two leaves and two internal nodes inactive inside active tiles"""
    parent = s.st.parent.copy()
    parent[np.array([2 * N_JOIN + 70, s.n - 3, s.n + 5, s.n + 130])] = s.st.maxnode - 1
    return parent


def _pattern_parent(s, counts, rng_seed):
    """`counts[i]` active leaves in span i, at random positions; the special leaves are among those of the last span"""
    rng = np.random.default_rng(rng_seed)
    parent = _base_parent(s)
    spec = _special(s.n)
    for i, cnt in enumerate(counts):
        lo, hi = i * SPAN, min((i + 1) * SPAN, s.n)
        ids = np.arange(lo, hi)
        parent[ids] = s.st.maxnode - 1
        keep = spec[(spec >= lo) & (spec < hi)]
        rest = np.setdiff1d(ids, keep)
        assert len(keep) <= cnt <= len(ids) or len(keep) == 0
        on = np.concatenate([keep, rng.choice(rest, cnt - len(keep), replace=False)]) if cnt else keep
        parent[on.astype(np.int64)] = -1
        assert (parent[ids] < 0).sum() == cnt
    return parent


def _set_parent(s, parent):
    s.ops.set_parents(0, parent)
    s.parent = parent
    s.active = np.nonzero(parent < 0)[0]
    s.k = len(s.active)


def _trio(shape, dt):
    return {opt: _make(shape, dt, opt) for opt in (PER_SEED, NO_MIXED, DEFAULT)}


def _close(t):
    for s in t.values():
        s.ops.close()


_TRIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for t in _TRIOS.values():
        _close(t)
    _TRIOS.clear()


def _get(shape, dt=np.float32):
    """the same state in three contexts: one launch per seed, per-kind passes only, the built-in choice; made once per module"""
    key = (shape, np.dtype(dt).name)
    if key not in _TRIOS:
        _TRIOS[key] = _trio(shape, dt)
    return _TRIOS[key]


@pytest.fixture(params=list(SHAPES))
def trio(request):
    t = _get(request.param)
    _reset(t)
    return t


@pytest.fixture
def trio64():
    return _get("n1300_L37", np.float64)


def _seeds(s, n_leaf, n_prof, rng_seed, special=0):
    """`special` of the leaf seeds are the first special leaves, the others random active leaves; shuffled among the profile seeds"""
    rng = np.random.default_rng(rng_seed)
    spec = _special(s.n)[:special]
    pool = np.setdiff1d(s.active[s.active < s.n], spec)
    leaves = np.concatenate([spec, rng.choice(pool, n_leaf - special, replace=False)])
    inner = rng.choice(s.active[s.active >= s.n], n_prof, replace=False)
    seeds = np.concatenate([leaves, inner]).astype(np.int64)
    rng.shuffle(seeds)
    return seeds


def _batch(s, seeds, k=None):
    st = s.st
    return s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, s.k if k is None else k)


def _compare(t, seeds, k=None, all_targets=True):
    got = {}
    for opt, s in t.items():
        hits, best = _batch(s, seeds, k)
        got[opt] = (hits, best, s.ops.sweep_results(0, s.st.maxnode))
    for ref in (PER_SEED, NO_MIXED):
        assert np.array_equal(got[DEFAULT][1], got[ref][1])
        assert np.array_equal(got[DEFAULT][0], got[ref][0])
        for a, b in zip(got[DEFAULT][2], got[ref][2]):
            assert np.array_equal(a, b)
    if all_targets:   # every active target is in every list, the inactive ones in none
        for h in got[DEFAULT][0]:
            assert np.array_equal(np.sort(h["j"]), t[DEFAULT].active)
    return got[DEFAULT]


def _launches(s, seeds):
    s.ops.timer_start()
    _batch(s, seeds)
    s.ops.timer_stop_ms()
    return s.ops.sweep_kernel_ms()[1], s.ops.sweep_kernel_sweeps()


def _patterns(t):
    s0 = t[DEFAULT]
    for i, counts in enumerate(PATTERNS[s0.shape]):
        parent = _pattern_parent(s0, counts, 1000 + i)
        for s in t.values():
            _set_parent(s, parent)
        yield counts


def _reset(t):
    for s in t.values():
        _set_parent(s, _base_parent(s))


def _with_special(s, which, inner_seed):
    """the special leaves `which` (indices into _special) as the four leaf seeds, in front of four random profile seeds"""
    rng = np.random.default_rng(inner_seed)
    inner = rng.choice(s.active[s.active >= s.n], 4, replace=False)
    return np.concatenate([_special(s.n)[list(which)], inner]).astype(np.int64)


def test_active_leaves_per_span(trio):
    """0, 1, 255, 256, 257, 512, 513 and 1024 active leaves in a span: a 4 + 4 batch with the four gap seeds, then one with the twins,
    against one launch per seed and the per-kind passes; one launch stands for the eight sweeps."""
    for i, counts in enumerate(_patterns(trio)):
        for which in ((0, 1, 2, 3), (4, 0, 5, 3)):
            seeds = _with_special(trio[DEFAULT], which, 10 + i)
            _compare(trio, seeds)
            assert _launches(trio[DEFAULT], seeds) == (1, 8), counts


@pytest.mark.parametrize("n_leaf,n_prof", [(4, 4), (5, 5), (4, 2)])
def test_seed_mixes(trio, n_leaf, n_prof):
    """4 + 4 (the mixed pass), 5 + 5 (singles beside it) and 4 + 2 (no mixed pass: per-kind groups), the gap seeds among the leaf seeds"""
    seeds = _seeds(trio[DEFAULT], n_leaf, n_prof, 100 * n_leaf + n_prof, special=4)
    _compare(trio, seeds)


def test_twin_seeds_get_equal_leaf_rows(trio):
    """two leaf seeds with the same sequence: the same distance and weight to every other leaf target (their criteria differ by the
    seeds' out-distances only)"""
    s = trio[DEFAULT]
    sp = _special(s.n)
    hits, _, _ = _compare(trio, _with_special(s, (4, 5, 0, 6), 5))
    a, b = (np.sort(hits[q][hits[q]["j"] < s.n], order="j") for q in (0, 1))
    assert np.array_equal(a["j"], b["j"])
    other = (a["j"] != sp[4]) & (a["j"] != sp[5])
    assert np.array_equal(a["dist"][other], b["dist"][other]) and np.array_equal(a["weight"][other], b["weight"][other])


def test_leaf_seeds_rotated_through_the_slots(trio):
    """the same four leaf seeds in each order of a rotation: every seed's list is what one launch per seed gives it"""
    s = trio[DEFAULT]
    base = _with_special(s, (0, 1, 2, 3), 6)
    for r in range(4):
        seeds = np.concatenate([np.roll(base[:4], r), base[4:]])
        _compare(trio, seeds)
        assert _launches(s, seeds) == (1, 8)


def test_launch_accounting(trio):
    """4 + 4: one launch for eight sweeps, two without the mixed pass, eight seed by seed"""
    seeds = _seeds(trio[DEFAULT], 4, 4, 3, special=2)
    for opt, want in ((DEFAULT, 1), (NO_MIXED, 2), (PER_SEED, 8)):
        assert _launches(trio[opt], seeds) == (want, 8)


def test_double_precision_is_unchanged(trio64):
    """double precision keeps the per-kind passes: two launches, the lists of one launch per seed"""
    seeds = _seeds(trio64[DEFAULT], 4, 4, 41, special=4)
    _compare(trio64, seeds)
    for opt, want in ((DEFAULT, 2), (NO_MIXED, 2), (PER_SEED, 8)):
        assert _launches(trio64[opt], seeds) == (want, 8)


def test_top_k_below_the_active_count(trio):
    """k = 50: k_select_hist reads the leaf seeds' min / max partials, numbered like a profile seed's now"""
    for _ in _patterns(trio):
        _compare(trio, _with_special(trio[DEFAULT], (2, 6, 4, 3), 57), k=50, all_targets=False)


def test_sharded_walk_merges_to_the_unsharded_lists(trio):
    """set_shard with lo a multiple of 64 but not of 1024, inside the leaves: the shard [lo, maxnode) takes the mixed pass with its
    spans counted from lo; the shards' top-k merged equal the unsharded top-k"""
    from veryfasttree_amd.workload import merge_hits
    s = trio[DEFAULT]
    st = s.st
    seeds = _seeds(s, 4, 4, 31, special=4)
    k = 200
    whole, best = s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)
    for split in (704, 1088):
        assert split % 64 == 0 and split % SPAN != 0 and split < s.n
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


def test_against_the_cpu_oracle():
    """the gap-in-column-16 leaf seed and one profile seed of a 4 + 4 batch against the reference restatement (tests/oracle.py):
    distance, weight and criterion of every active target, bit for bit"""
    from oracle import Oracle
    t = _get("n1300_L37")
    _reset(t)
    s = t[DEFAULT]
    ops, st = s.ops, s.st
    orc = Oracle(ops.dt)
    profs = [ops.profile_download(int(i)) for i in range(st.maxnode)]
    W = np.stack([p[0] for p in profs]); Cc = np.stack([p[1] for p in profs]); F = np.stack([p[2] for p in profs])
    diam, selfw, selfd = ops.get_node_scalars(0, st.maxnode)
    od, na = ops.get_out_distances(0, st.maxnode)
    assert np.all(na[s.active] == st.n_active)   # nothing stale: the oracle's lazy refresh has nothing to do either
    outp, _ = orc.out_profile(W[s.active], Cc[s.active], F[s.active])
    ost = orc.state(s.n, W, Cc, F, s.parent, diam, selfw, selfd, st.totdiam, outp)
    seeds = _with_special(s, (2, 0, 1, 3), 23)
    hits, best = _batch(s, seeds)
    for slot in (0, 4):
        exp = orc.set_best_hit(ost, int(seeds[slot]), st.n_active, st.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
