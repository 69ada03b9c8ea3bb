"""In single precision the internal-target column loops of k_sweep_nt_mixed_multi and k_sweep_nt_profq_multi pick f_t[c] for a seed's
wave-uniform code c with the VGPR index mode - one indexed v_cvt_f64_f32 per (seed, column), the index the low two bits of the seed's
byte in the column's code record (vft_isel_cvt in csrc/vft_kernels_nj.h) - where two masks and three selects did it before.  The value
is the same float, so every bit must stay where it was.  What can go wrong is the index: the wrong byte of the record, a stale M0, a
read outside the column's four registers - so every code 0..3 and NOCODE is put at every byte position of both records (the leaf
seeds' dword per column, the profile seeds' code dword), in column 0, in the first and the last column of a group, and in the last
real column.

The same state in three contexts, as in test_gpu_seed_code_records.py: one launch per seed (the single-seed kernels know no index
mode), the per-kind passes, and the built-in choice.  k = the number of active nodes.  384 leaf rows, 96 sibling pairs joined.

    L = 37    the last group (32..39) is part padding
    L = 60    the last group (56..63) holds four real columns
    L = 130   columns 136..143 are a pure padding group

Crafted LEAF seeds: CONST[c] (code c in every column), CYCLE (code p % 4 in column p), GAPS (random codes; gaps in column 0, in the
first and last column of groups 0, 1 and the last one, and in the last real column).
Crafted PROFILE seeds: CYC[r] (identical children with code (p + r) % 4: every column plain, the four of them hold all four codes in
every column), DIFFER (children differ in every column: every byte NOCODE, the vector arm), HALFGAP (one child gapped in every third
column: plain codes below weight 1), BOTHGAP (gap columns, plain codes, weights 1/2, vectors).
The four rotations of a group of four put each seed into every byte q = 0..3 of its record.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, N_JOIN = 384, 96
SHAPES = {"L37": (37, 31), "L60": (60, 32), "L130": (130, 33)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)
CYC = (10, 11, 12, 13)   # the crafted pairs (internal nodes N + pair)
DIFFER, HALFGAP, BOTHGAP = 20, 21, 22
CONST = (200, 263, 300, 383)   # the crafted leaf seeds, in all three active leaf tiles
CYCLE, GAPS = 210, 320
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
    a, b = base.copy(), base.copy()
    b[0::5] = (base[0::5] + 1) % 4     # differing
    a[2::5] = b[2::5] = NOCODE         # gapped in both
    a[3::5] = NOCODE                   # gapped in one
    codes[2 * BOTHGAP], codes[2 * BOTHGAP + 1] = a, b
    for c, row in enumerate(CONST):
        codes[row] = c
    codes[CYCLE] = p % 4
    codes[GAPS] = rng.integers(0, 4, L)
    codes[GAPS, 2:6] = np.arange(4)   # all four codes, whatever the draw
    codes[GAPS, _gap_columns(L)] = NOCODE


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
    s.leaf_groups = [np.array(CONST, np.int64), np.array([CYCLE, GAPS, CONST[3], CONST[0]], np.int64)]
    s.prof_groups = [np.array([N + c for c in CYC], np.int64), np.array([N + DIFFER, N + HALFGAP, N + BOTHGAP, N + CYC[1]], np.int64)]
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
    got = {n: s.ops.profile_download(N + n)[1][:L] for n in CYC + (DIFFER, HALFGAP, BOTHGAP)}
    for r, n in enumerate(CYC):
        assert np.array_equal(got[n], (np.arange(L) + r) % 4)
    assert np.all(got[DIFFER] == NOCODE)
    w = s.ops.profile_download(N + HALFGAP)[0][:L]
    assert np.all(got[HALFGAP] == (np.arange(L) + 2) % 4) and np.all(w[1::3] < 1) and np.all(w[0::3] == 1)
    assert np.any(got[BOTHGAP] == NOCODE) and np.any(got[BOTHGAP] != NOCODE)
    # so in every column the four CYC seeds hold the four codes, and a rotation of the group moves each into every byte
    assert all(set(got[n][p] for n in CYC) == {0, 1, 2, 3} for p in (0, 7, 8, L - 1))
    # the internal targets: plain columns, columns with an explicit weight, vector columns
    plain = weighted = vector = 0
    for j in s.active[s.active >= N]:
        w, code, f = s.ops.profile_download(int(j))
        w, code = w[:L], code[:L]
        plain += int(np.sum((code != NOCODE) & (w == 1)))
        weighted += int(np.sum((code != NOCODE) & (w > 0) & (w < 1)))
        vector += int(np.sum((code == NOCODE) & (w > 0)))
    assert plain > 0 and weighted > 0 and vector > 0


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


@pytest.mark.parametrize("rot", range(4))
@pytest.mark.parametrize("group", [0, 1])
def test_four_leaf_seeds_alone(trio, group, rot):
    """4 + 0: k_sweep_nt_leafq_multi<4> (which keeps the selects: its 70 registers have no room for 32 fixed ones)"""
    _same_everywhere(trio, np.roll(trio[DEFAULT].leaf_groups[group], rot), {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("pair", [(CYCLE, GAPS), (GAPS, CONST[2]), (CONST[1], CYCLE), (CONST[3], CONST[0])])
def test_two_leaf_seeds(trio, pair):
    """2 + 0: k_sweep_nt_leafq_multi<2> - bytes 2 and 3 of the record belong to no seed"""
    _same_everywhere(trio, np.array(pair, np.int64), {DEFAULT: 1, NO_MIXED: 1})


@pytest.mark.parametrize("pair", [(CYC[0], DIFFER), (BOTHGAP, CYC[3]), (CYC[2], CYC[1]), (HALFGAP, BOTHGAP)])
def test_two_profile_seeds(trio, pair):
    """0 + 2: k_sweep_nt_profq_multi<2> - the two-seed form of the indexed read"""
    _same_everywhere(trio, np.array([N + p for p in pair], np.int64), {DEFAULT: 1, NO_MIXED: 1})


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


def test_one_seed_of_each_kind_against_the_cpu_oracle(trio, oracle_state):
    """GAPS and BOTHGAP, out of a 4 + 4 batch, against the reference restatement: distance, weight and criterion of every active
    target, bit for bit"""
    s = trio[DEFAULT]
    st = s.st
    orc, ost, od, na = oracle_state
    seeds = np.concatenate([s.leaf_groups[1], s.prof_groups[1]])
    hits, best = _batch(s, seeds)
    for slot in (1, 6):
        assert int(seeds[slot]) in (GAPS, N + BOTHGAP)
        exp = orc.set_best_hit(ost, int(seeds[slot]), st.n_active, st.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
