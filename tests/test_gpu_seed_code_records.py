"""Leaf seeds of a multi-seed pass read their codes from the group's code record (a dword per column, a byte per seed), the uniform
selects of both kinds of seed take their lane masks from single bits of the code bytes, and a leaf seed's gap skips the pair
(vft_int_chunk_consume_all, vft_int_chunk_consume_prof in csrc/vft_kernels_nj.h).  All of it must leave every bit where it was.

The same state in three contexts, as in test_gpu_mixed_pass.py: one launch per seed (the single-seed kernels know none of this), the
per-kind passes (k_sweep_nt_leafq_multi, k_sweep_nt_profq_multi) and the built-in choice (k_sweep_nt_mixed_multi in single precision).
k = the number of active nodes: the hit lists hold the distance, weight and criterion of every active target.

384 leaf rows: 96 sibling pairs (rows 0..191) are joined, rows 192..383 stay active leaves - three tiles of 64 leaf ids that hold active
targets, and the 96 internal ids 384..479 in two tiles.

    L = 37    the last group (32..39) is part padding
    L = 60    the last group (56..63) holds four real columns
    L = 130   columns 136..143 are a pure padding group, and L is above VFT_PTILE_M

Crafted LEAF seeds (rows overwritten before the upload; every row but ALLGAP holds all four codes):
    GAP0      a gap in column 0
    GAPLAST   a gap in the last real column
    GAPGROUP  columns 8..15, a whole group of 8, gapped
    ALLGAP    nothing but gaps: denom 0 against every internal target, so distance 1.0 and weight 0.01
and all four are gapped in column 20.  The four rotations of the group put each of them - so all four codes, and each gap pattern - into
every byte q = 0..3 of the record.  Crafted PROFILE seeds as in test_gpu_plain_query_columns.py: SAME (every column plain), DIFFER (none),
HALFGAP (plain codes below weight 1), BOTHGAP (gap columns, plain codes, weights 1/2, vectors).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, N_JOIN = 384, 96
SHAPES = {"L37": (37, 21), "L60": (60, 22), "L130": (130, 23)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)
SAME, DIFFER, HALFGAP, BOTHGAP = 10, 11, 12, 13   # the crafted pairs (internal nodes N + pair)
GAP0, GAPLAST, GAPGROUP, ALLGAP = 200, 263, 300, 383   # the crafted leaf seeds, in all three active leaf tiles
NOCODE = 127


class _State:
    pass


def _craft(codes, L, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, L).astype(codes.dtype)
    codes[2 * SAME] = codes[2 * SAME + 1] = base
    codes[2 * DIFFER] = base
    codes[2 * DIFFER + 1] = (base + 1 + rng.integers(0, 3, L)) % 4
    codes[2 * HALFGAP] = codes[2 * HALFGAP + 1] = base
    codes[2 * HALFGAP + 1, 1::3] = NOCODE
    a, b = base.copy(), base.copy()
    b[0::5] = (base[0::5] + 1) % 4     # differing
    a[2::5] = b[2::5] = NOCODE         # gapped in both
    a[3::5] = NOCODE                   # gapped in one
    codes[2 * BOTHGAP], codes[2 * BOTHGAP + 1] = a, b
    for row in (GAP0, GAPLAST, GAPGROUP):
        codes[row] = rng.integers(0, 4, L)
        codes[row, 2:6] = np.roll(np.arange(4), row % 4)   # all four codes, whatever the draw
    codes[GAP0, 0] = NOCODE
    codes[GAPLAST, L - 1] = NOCODE
    codes[GAPGROUP, 8:16] = NOCODE
    codes[ALLGAP] = NOCODE
    codes[[GAP0, GAPLAST, GAPGROUP], 20] = NOCODE


def _make(shape, dt, option):
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.workload import TopHitsState
    L, seed = SHAPES[shape]
    codes = synth.random_descent_codes(N, L, 4, 0.05, 0.1, seed=seed)
    _craft(codes, L, seed)
    ops = HipProfileOps(N, L, 4, dt)
    assert ops.lib.vft_debug_option(ops.ctx, ctypes.c_int32(12), ctypes.c_int64(option)) == 0
    st = TopHitsState(ops, codes, N_JOIN)
    # inactive nodes in otherwise active tiles: two leaves behind the joined ones, two internal nodes
    off = np.array([2 * N_JOIN + 70, N - 3, N + 5, N + 70])
    parent = st.parent.copy()
    parent[off] = st.maxnode - 1
    ops.set_parents(0, parent)
    s = _State()
    s.ops, s.st, s.L, s.codes, s.parent = ops, st, L, codes, parent
    s.active = np.nonzero(parent < 0)[0]
    s.k = len(s.active)
    s.leaf_seeds = np.array([GAP0, GAPLAST, GAPGROUP, ALLGAP], np.int64)
    s.prof_seeds = np.array([N + SAME, N + DIFFER, N + HALFGAP, N + BOTHGAP], np.int64)
    assert np.all(parent[s.leaf_seeds] < 0) and np.all(parent[s.prof_seeds] < 0)
    return s


@pytest.fixture(scope="module", params=[(sh, dt) for sh in SHAPES for dt in (np.float32, np.float64)],
                ids=lambda p: "%s-%s" % (p[0], np.dtype(p[1]).name))
def trio(request):
    shape, dt = request.param
    t = {opt: _make(shape, dt, opt) for opt in (PER_SEED, NO_MIXED, DEFAULT)}
    yield t
    for s in t.values():
        s.ops.close()


def _batch(s, seeds):
    st = s.st
    return s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, s.k)


def _same_everywhere(trio, seeds, launches):
    """the batch in the three contexts: equal hit lists, bestJ and slot 0's result arrays - and the built-in path took `launches`
    launches for len(seeds) sweeps (a fallback to one launch per seed would compare the single-seed kernels with themselves)"""
    got = {}
    for opt, s in trio.items():
        s.ops.timer_start()
        hits, best = _batch(s, seeds)
        s.ops.timer_stop_ms()
        assert s.ops.sweep_kernel_sweeps() == len(seeds)
        assert s.ops.sweep_kernel_ms()[1] == (len(seeds) if opt == PER_SEED else launches[opt])
        got[opt] = (hits, best, s.ops.sweep_results(0, s.st.maxnode))
    for ref in (PER_SEED, NO_MIXED):
        assert np.array_equal(got[DEFAULT][1], got[ref][1])
        assert np.array_equal(got[DEFAULT][0], got[ref][0])
        for a, b in zip(got[DEFAULT][2], got[ref][2]):
            assert np.array_equal(a, b)
    for h in got[DEFAULT][0]:
        assert np.array_equal(np.sort(h["j"]), trio[DEFAULT].active)
    return got[DEFAULT]


def test_the_crafted_leaves_are_what_they_are_meant_to_be(trio):
    s = trio[DEFAULT]
    c = s.codes
    assert c[GAP0, 0] == NOCODE and c[GAPLAST, s.L - 1] == NOCODE and np.all(c[GAPGROUP, 8:16] == NOCODE) and np.all(c[ALLGAP] == NOCODE)
    assert np.all(c[s.leaf_seeds, 20] == NOCODE)
    for row in (GAP0, GAPLAST, GAPGROUP):
        assert set(c[row][c[row] != NOCODE]) == {0, 1, 2, 3}
    w, code, f = s.ops.profile_download(ALLGAP)
    assert np.all(code == NOCODE) and np.all(w == 0)


@pytest.mark.parametrize("rot", range(4))
def test_four_crafted_leaf_and_four_crafted_profile_seeds(trio, rot):
    """4 + 4: the mixed pass in single precision, the two per-kind passes in double precision and under option 8"""
    s = trio[DEFAULT]
    f32 = s.ops.dt == np.float32
    seeds = np.concatenate([np.roll(s.leaf_seeds, rot), np.roll(s.prof_seeds, rot)])
    hits, best, res = _same_everywhere(trio, seeds, {DEFAULT: 1 if f32 else 2, NO_MIXED: 2})
    # the seed without a column: denom 0, so weight 0.01 against every internal target (the distance, 1.0, carries the diameters)
    h = hits[int(np.nonzero(seeds == ALLGAP)[0][0])]
    assert np.all(h["weight"][h["j"] >= N] == s.ops.dt.type(0.01))
    # slot 0 a profile seed: its result arrays are the ones sweep_results reads
    _same_everywhere(trio, seeds[::-1].copy(), {DEFAULT: 1 if f32 else 2, NO_MIXED: 2})


@pytest.mark.parametrize("rot", range(4))
def test_four_crafted_leaf_seeds_alone(trio, rot):
    """4 + 0: k_sweep_nt_leafq_multi<4> in both precisions"""
    _same_everywhere(trio, np.roll(trio[DEFAULT].leaf_seeds, rot), {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("rot", range(4))
def test_four_crafted_profile_seeds_alone(trio, rot):
    """0 + 4: k_sweep_nt_profq_multi<4> in both precisions"""
    _same_everywhere(trio, np.roll(trio[DEFAULT].prof_seeds, rot), {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("pair", [(GAP0, ALLGAP), (ALLGAP, GAPGROUP), (GAPLAST, GAP0), (GAPGROUP, GAPLAST)])
def test_two_crafted_leaf_seeds(trio, pair):
    """2 + 0: k_sweep_nt_leafq_multi<2> - bytes 2 and 3 of the record belong to no seed"""
    _same_everywhere(trio, np.array(pair, np.int64), {DEFAULT: 1, NO_MIXED: 1})


@pytest.fixture(scope="module")
def oracle_state(trio):
    """the reference restatement's view of the state (tests/oracle.py), made once per shape and precision"""
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
    return orc, orc.state(N, W, Cc, F, s.parent, diam, selfw, selfd, st.totdiam, outp), od, na


@pytest.mark.parametrize("batch", ["4+4", "4+0", "2+0"])
def test_crafted_seeds_against_the_cpu_oracle(trio, oracle_state, batch):
    """every seed of the batch against the reference restatement: distance, weight and criterion of every active target, bit for bit"""
    s = trio[DEFAULT]
    st = s.st
    orc, ost, od, na = oracle_state
    seeds = {"4+4": np.concatenate([np.roll(s.leaf_seeds, 1), s.prof_seeds]), "4+0": np.roll(s.leaf_seeds, 2),
             "2+0": np.array([ALLGAP, GAPGROUP], np.int64)}[batch]
    hits, best = _batch(s, seeds)
    for slot in range(len(seeds)):
        exp = orc.set_best_hit(ost, int(seeds[slot]), st.n_active, st.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
