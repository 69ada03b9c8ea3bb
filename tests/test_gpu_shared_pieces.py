"""In single precision the internal-target column loops of k_sweep_nt_mixed_multi and k_sweep_nt_profq_multi compute the four pieces
1 - f_t[k] of a target's column once, into four fixed register pairs, and every seed's product w * piece reads its piece by the VGPR
index mode (vft_ipiece_mul / vft_int_chunk_consume_shared in csrc/vft_kernels_nj.h); the mixed kernel finishes a column's profile
seeds and leaf seeds before the next column.  Every floating-point operation per (seed, target) is the one it was, so every bit must
stay where it was.  What can go wrong, and what test_gpu_gpr_index_select.py does not pin:

  - a wrong or stale index into the pieces.  A two-leaf average only holds 0, 1/2 and 1, so swapped indices can hide: DEEP targets
    (three levels of averages over eight leaves, in the free id space) have columns whose four frequencies are pairwise different -
    at every one of the eight positions of a group;
  - the index taken from the wrong byte of a record: seeds that hold all four codes in every column (CYC, CONST, CYCLE), rotated
    through the four slots;
  - a leaf seed's gap: its indexed product must be discarded (column 0, first and last column of a group, last real column);
  - the vector arm: on every column (DIFFER), on every other column (ALT: the arm overrides that seed's indexed product and nobody
    else's), and not at all at a weight below 1 (HALFGAP);
  - 4 + 4, 0 + 4, 0 + 2 and 4 + 0 seeds.

The same state in three contexts, as in test_gpu_gpr_index_select.py: one launch per seed (the single-seed kernels share nothing), the
per-kind passes, and the built-in choice.  k = the number of active nodes.  384 leaf rows, 96 sibling pairs joined, 16 x 7 deep nodes.

    L = 37    the last group (32..39) is part padding
    L = 60    the last group (56..63) holds four real columns
    L = 130   columns 136..143 are a pure padding group
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, N_JOIN, N_DEEP = 384, 96, 16
BASE = N + N_JOIN                       # the deep nodes: level 3 at BASE, level 2 behind it, level 1 last
SHAPES = {"L37": (37, 41), "L60": (60, 42), "L130": (130, 43)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)
CYC = (10, 11, 12, 13)                  # the crafted pairs (internal nodes N + pair)
DIFFER, HALFGAP, ALT = 20, 21, 22
CONST = (200, 263, 300, 383)            # the crafted leaf seeds, in all three active leaf tiles
CYCLE, GAPS = 210, 320
DEEP0 = np.arange(96, 104)              # the eight leaves under deep node BASE: counts 4, 3, 1, 0 of the four codes in every column
NOCODE = 127


class _State:
    pass


def _gap_columns(L):
    last = (L - 1) // 8 * 8
    return sorted({0, 7, 8, 15, last, L - 1})


def _craft(codes, L, seed):
    rng = np.random.default_rng(seed)
    p = np.arange(L)
    for r, pair in enumerate(CYC):
        codes[2 * pair] = codes[2 * pair + 1] = (p + r) % 4
    base = rng.integers(0, 4, L).astype(codes.dtype)
    codes[2 * DIFFER] = base
    codes[2 * DIFFER + 1] = (base + 1 + rng.integers(0, 3, L)) % 4
    codes[2 * HALFGAP] = codes[2 * HALFGAP + 1] = (p + 2) % 4
    codes[2 * HALFGAP + 1, 1::3] = NOCODE
    codes[2 * ALT] = codes[2 * ALT + 1] = (p + 1) % 4
    codes[2 * ALT + 1, 1::2] = (codes[2 * ALT, 1::2] + 1 + rng.integers(0, 3, len(p[1::2]))) % 4   # odd columns: a vector
    for c, row in enumerate(CONST):
        codes[row] = c
    codes[CYCLE] = p % 4
    codes[GAPS] = rng.integers(0, 4, L)
    codes[GAPS, 2:6] = np.arange(4)   # all four codes, whatever the draw
    codes[GAPS, _gap_columns(L)] = NOCODE
    # eight leaves whose average has the frequencies 4/8, 3/8, 1/8 and 0 - which code has which changes from column to column
    for i, leaf in enumerate(DEEP0):
        codes[leaf] = ((0, 0, 0, 0, 1, 1, 1, 2)[i] + p + p // 4) % 4


def _deep_nodes(ops, st, seed):
    """N_DEEP groups of eight leaves averaged over three levels (as bench.py's dense profiles), all 7 N_DEEP nodes active targets"""
    rng = np.random.default_rng(seed)
    free = np.setdiff1d(np.arange(N), DEEP0)
    leaves = np.concatenate([DEEP0, rng.permutation(free)[:8 * (N_DEEP - 1)]]).astype(np.int64)
    l3 = BASE + np.arange(N_DEEP, dtype=np.int64)
    l2 = BASE + N_DEEP + np.arange(2 * N_DEEP, dtype=np.int64)
    l1 = BASE + 3 * N_DEEP + np.arange(4 * N_DEEP, dtype=np.int64)
    maxnode = BASE + 7 * N_DEEP
    assert maxnode <= ops.max_nodes
    ops.set_max_node(maxnode)
    for out, a, b in ((l1, leaves[0::2], leaves[1::2]), (l2, l1[0::2], l1[1::2]), (l3, l2[0::2], l2[1::2])):
        ops.averageProfile(out, a, b)
    ops.set_node_scalars(BASE, diameter=(0.01 + 0.05 * rng.random(7 * N_DEEP)).astype(ops.dt))
    return maxnode


def _make(shape, dt, option):
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.workload import TopHitsState
    L, seed = SHAPES[shape]
    codes = synth.random_descent_codes(N, L, 4, 0.05, 0.1, seed=seed)
    _craft(codes, L, seed)
    ops = HipProfileOps(N, L, 4, dt)
    assert ops.lib.vft_debug_option(ops.ctx, ctypes.c_int32(12), ctypes.c_int64(option)) == 0
    st = TopHitsState(ops, codes, N_JOIN)
    maxnode = _deep_nodes(ops, st, seed)
    parent = np.full(maxnode, -1, np.int64)
    parent[:st.maxnode] = st.parent
    # inactive nodes in otherwise active tiles: two leaves behind the joined ones, two pair nodes, two deep nodes
    parent[np.array([2 * N_JOIN + 70, N - 3, N + 5, N + 70, BASE + 3, BASE + 60])] = maxnode - 1
    ops.set_parents(0, parent)
    s = _State()
    s.ops, s.st, s.L, s.codes, s.parent, s.maxnode = ops, st, L, codes, parent, maxnode
    s.active = np.nonzero(parent < 0)[0]
    s.k = s.n_active = len(s.active)
    s.n_diff_allow = int(s.n_active * 0.01)
    ops.outProfile(s.active)
    ops.set_out_distances(0, np.zeros(maxnode, dt), np.full(maxnode, 10 * N, np.int64))
    ops.setOutDistance(None, s.n_active, st.totdiam)
    ops.synchronize()
    s.leaf_groups = [np.array(CONST, np.int64), np.array([CYCLE, GAPS, CONST[3], CONST[0]], np.int64)]
    s.prof_groups = [np.array([N + c for c in CYC], np.int64), np.array([N + DIFFER, N + HALFGAP, N + ALT, N + CYC[1]], np.int64)]
    for g in s.leaf_groups + s.prof_groups:
        assert np.all(parent[g] < 0)
    return s


@pytest.fixture(scope="module", params=[("L37", np.float32), ("L60", np.float32), ("L130", np.float32), ("L60", np.float64)],
                ids=lambda p: "%s-%s" % (p[0], np.dtype(p[1]).name))
def trio(request):
    shape, dt = request.param
    t = {opt: _make(shape, dt, opt) for opt in (PER_SEED, NO_MIXED, DEFAULT)}
    yield t
    for s in t.values():
        s.ops.close()


def _batch(s, seeds):
    return s.ops.setBestHitBatch(seeds, s.n_active, s.n_diff_allow, s.st.totdiam, s.k)


def _same_everywhere(trio, seeds, launches):
    """the batch in the three contexts: equal hit records, bestJ and slot 0's result arrays, bit for bit - and the built-in path took
    `launches` launches for len(seeds) sweeps (a fallback to one launch per seed would compare the single-seed kernels with themselves)"""
    got = {}
    for opt, s in trio.items():
        s.ops.timer_start()
        hits, best = _batch(s, seeds)
        s.ops.timer_stop_ms()
        assert s.ops.sweep_kernel_sweeps() == len(seeds)
        assert s.ops.sweep_kernel_ms()[1] == (len(seeds) if opt == PER_SEED else launches[opt])
        got[opt] = (hits, best, s.ops.sweep_results(0, s.maxnode))
    for ref in (PER_SEED, NO_MIXED):
        assert np.array_equal(got[DEFAULT][1], got[ref][1])
        assert got[DEFAULT][0].tobytes() == got[ref][0].tobytes()
        for a, b in zip(got[DEFAULT][2], got[ref][2]):
            assert a.tobytes() == b.tobytes()
    for h in got[DEFAULT][0]:
        assert np.array_equal(np.sort(h["j"]), trio[DEFAULT].active)
    return got[DEFAULT]


def test_the_crafted_seeds_and_the_targets_are_what_they_are_meant_to_be(trio):
    s = trio[DEFAULT]
    c, L = s.codes, s.L
    cols = _gap_columns(L)
    assert {0, 7, 8, 15, L - 1} <= set(cols) and (L - 1) // 8 * 8 in cols
    assert np.all(c[GAPS, cols] == NOCODE) and set(c[GAPS][c[GAPS] != NOCODE]) == {0, 1, 2, 3}
    for code, row in enumerate(CONST):
        assert np.all(c[row] == code)
    assert np.array_equal(c[CYCLE], np.arange(L) % 4)
    # the profile seeds' code bytes, as the kernel's record holds them (vft_extract_query copies the profile's codes)
    got = {n: s.ops.profile_download(N + n)[1][:L] for n in CYC + (DIFFER, HALFGAP, ALT)}
    for r, n in enumerate(CYC):
        assert np.array_equal(got[n], (np.arange(L) + r) % 4)
    assert np.all(got[DIFFER] == NOCODE)
    w = s.ops.profile_download(N + HALFGAP)[0][:L]
    assert np.all(got[HALFGAP] == (np.arange(L) + 2) % 4) and np.all(w[1::3] < 1) and np.all(w[0::3] == 1)
    assert np.all(got[ALT][0::2] == (np.arange(L)[0::2] + 1) % 4) and np.all(got[ALT][1::2] == NOCODE)
    # so in every column the four CYC seeds hold the four codes, and a rotation of the group moves each into every byte
    assert all(set(got[n][p] for n in CYC) == {0, 1, 2, 3} for p in range(L))
    # the deep targets: at each of the eight positions of a group a column whose four frequencies are pairwise different
    distinct = np.zeros(L, bool)
    for j in s.active[s.active >= BASE]:
        w, code, f = s.ops.profile_download(int(j))
        f = np.asarray(f).reshape(-1, 4)[:L]
        vec = (np.asarray(code)[:L] == NOCODE) & (np.asarray(w)[:L] > 0)
        distinct |= vec & np.array([len(set(row.tolist())) == 4 for row in f])
    for b in range(8):
        assert np.any(distinct[b::8]), "no target column with four different frequencies at position %d of a group" % b
    wf = s.ops.profile_download(BASE)
    assert sorted(np.asarray(wf[2]).reshape(-1, 4)[0].tolist()) == [0.0, 0.125, 0.375, 0.5]


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("group", [0, 1])
def test_four_leaf_and_four_profile_seeds(trio, group, rot):
    """4 + 4: the mixed pass in single precision, the two per-kind passes in double precision and under option 8"""
    s = trio[DEFAULT]
    f32 = s.ops.dt == np.float32
    seeds = np.concatenate([np.roll(s.leaf_groups[group], rot), np.roll(s.prof_groups[group], rot)])
    _same_everywhere(trio, seeds, {DEFAULT: 1 if f32 else 2, NO_MIXED: 2})
    if rot == 0:   # slot 0 a profile seed: its result arrays are the ones sweep_results reads
        _same_everywhere(trio, seeds[::-1].copy(), {DEFAULT: 1 if f32 else 2, NO_MIXED: 2})


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("group", [0, 1])
def test_four_profile_seeds_alone(trio, group, rot):
    """0 + 4: k_sweep_nt_profq_multi<4>"""
    _same_everywhere(trio, np.roll(trio[DEFAULT].prof_groups[group], rot), {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("group", [0, 1])
def test_four_leaf_seeds_alone(trio, group):
    """4 + 0: k_sweep_nt_leafq_multi<4>, which shares nothing (no registers for a fixed block) - unchanged"""
    _same_everywhere(trio, trio[DEFAULT].leaf_groups[group], {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("pair", [(CYC[0], DIFFER), (ALT, CYC[3]), (CYC[2], CYC[1]), (HALFGAP, ALT)])
def test_two_profile_seeds(trio, pair):
    """0 + 2: k_sweep_nt_profq_multi<2> - the two-seed form of the indexed product"""
    _same_everywhere(trio, np.array([N + p for p in pair], np.int64), {DEFAULT: 1, NO_MIXED: 1})


@pytest.fixture(scope="module")
def oracle_state(trio):
    """the reference restatement's view of the state (tests/oracle.py), made once per shape and precision"""
    from oracle import Oracle
    s = trio[DEFAULT]
    ops = s.ops
    orc = Oracle(ops.dt)
    profs = [ops.profile_download(int(i)) for i in range(s.maxnode)]
    W = np.stack([p[0] for p in profs]); Cc = np.stack([p[1] for p in profs]); F = np.stack([p[2] for p in profs])
    diam, selfw, selfd = ops.get_node_scalars(0, s.maxnode)
    od, na = ops.get_out_distances(0, s.maxnode)
    assert np.all(na[s.active] == s.n_active)   # nothing stale: the oracle's lazy refresh has nothing to do either
    outp, _ = orc.out_profile(W[s.active], Cc[s.active], F[s.active])
    return orc, orc.state(N, W, Cc, F, s.parent, diam, selfw, selfd, s.st.totdiam, outp), od, na


def test_one_seed_of_each_kind_against_the_cpu_oracle(trio, oracle_state):
    """GAPS and ALT, out of a 4 + 4 batch, against the reference restatement: distance, weight and criterion of every active target,
    the deep ones included, bit for bit"""
    s = trio[DEFAULT]
    orc, ost, od, na = oracle_state
    seeds = np.concatenate([s.leaf_groups[1], s.prof_groups[1]])
    hits, best = _batch(s, seeds)
    for slot in (1, 6):
        assert int(seeds[slot]) in (GAPS, N + ALT)
        exp = orc.set_best_hit(ost, int(seeds[slot]), s.n_active, s.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
