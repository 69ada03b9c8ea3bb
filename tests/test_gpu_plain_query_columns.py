"""Profile seeds whose columns are plain codes: vft_int_chunk_consume_prof takes the leaf-seed arithmetic there (1 - f_t[c]) and the
multi-seed column loops skip a group of 8 columns that is pure padding.  Both must leave every bit where it was.

The same state in three contexts, as in test_gpu_mixed_pass.py: one launch per seed (k_sweep_nt / k_sweep_nt_both / k_sweep_nt_table,
which know nothing of either change), the per-kind passes (k_sweep_nt_profq_multi, k_sweep_nt_leafq_multi) and the built-in choice
(k_sweep_nt_mixed_multi in single precision).  k = the number of active nodes: the hit lists hold every target.

    n = 1300, L = 37    columns 40..47 are a pure padding group
    n = 1344, L = 130   columns 136..143 are one, and L is above VFT_PTILE_M
    n = 1300, L = 60    the last group (56..63) holds four real columns: nothing to skip

Crafted sibling pairs (leaf rows overwritten before the upload; node n + p is the average of leaves 2p and 2p + 1):
    SAME     identical leaves without a gap          every column of the profile a plain code, weight 1
    DIFFER   the leaves differ in every column       no plain column: 37 / 130 / 60 vectors
    HALFGAP  identical, one leaf gapped in a third   plain codes with weight 1/2 there
    BOTHGAP  some columns gapped in both, some in one, some differing      gap columns (weight 0), plain codes, weights 1/2, vectors
Each of them sits in every slot 0..3 of the profile group (the four rotations of the group).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_JOIN = 300
SHAPES = {"n1300_L37": (1300, 37, 11), "n1344_L130": (1344, 130, 12), "n1300_L60": (1300, 60, 13)}
PER_SEED, NO_MIXED, DEFAULT = 1, 8, 0   # values of VFT_DEBUG_NO_MULTI_SWEEP (vft_debug_option 12)
SAME, DIFFER, HALFGAP, BOTHGAP = 10, 11, 12, 13   # the crafted pairs
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


def _make(shape, dt, option):
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.workload import TopHitsState
    n, L, seed = SHAPES[shape]
    codes = synth.random_descent_codes(n, L, 4, 0.05, 0.1, seed=seed)
    _craft(codes, L, seed)
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
    s.crafted = np.array([n + SAME, n + DIFFER, n + HALFGAP, n + BOTHGAP], np.int64)
    return s


@pytest.fixture(scope="module", params=[(sh, dt) for sh in SHAPES for dt in (np.float32, np.float64)],
                ids=lambda p: "%s-%s" % (p[0], np.dtype(p[1]).name))
def trio(request):
    shape, dt = request.param
    t = {opt: _make(shape, dt, opt) for opt in (PER_SEED, NO_MIXED, DEFAULT)}
    yield t
    for s in t.values():
        s.ops.close()


def _leaf_seeds(s, rng_seed):
    rng = np.random.default_rng(rng_seed)
    return rng.choice(s.active[s.active < s.n], 4, replace=False)


def _batch(s, seeds):
    st = s.st
    return s.ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, s.k)


def _same_everywhere(trio, seeds):
    got = {}
    for opt, s in trio.items():
        hits, best = _batch(s, seeds)
        got[opt] = (hits, best, s.ops.sweep_results(0, s.st.maxnode))
    for ref in (PER_SEED, NO_MIXED):
        assert np.array_equal(got[DEFAULT][1], got[ref][1])
        assert np.array_equal(got[DEFAULT][0], got[ref][0])
        for a, b in zip(got[DEFAULT][2], got[ref][2]):
            assert np.array_equal(a, b)
    for h in got[DEFAULT][0]:
        assert np.array_equal(np.sort(h["j"]), trio[DEFAULT].active)
    return got[DEFAULT]


def test_the_crafted_profiles_are_what_they_are_meant_to_be(trio):
    s = trio[DEFAULT]
    one = s.ops.dt.type(1)

    def below_one(x):
        return np.all((x > 0) & (x < one))
    w, c, f = s.ops.profile_download(int(s.n + SAME))
    assert np.all(c != NOCODE) and np.all(w == one)
    w, c, f = s.ops.profile_download(int(s.n + DIFFER))
    assert np.all(c == NOCODE) and np.all(w == one)
    w, c, f = s.ops.profile_download(int(s.n + HALFGAP))
    assert np.all(c != NOCODE) and below_one(w[1::3]) and np.all(np.delete(w, np.s_[1::3]) == one)
    w, c, f = s.ops.profile_download(int(s.n + BOTHGAP))
    assert np.all(w[2::5] == 0) and np.all(c[2::5] == NOCODE)            # gap columns
    assert below_one(w[3::5]) and np.all(c[3::5] != NOCODE)         # plain codes below weight 1
    assert np.all(w[0::5] == one) and np.all(c[0::5] == NOCODE)          # vectors
    assert np.all(w[1::5] == one) and np.all(c[1::5] != NOCODE)


@pytest.mark.parametrize("rot", range(4))
def test_four_leaf_and_four_crafted_profile_seeds(trio, rot):
    """4 + 4: the mixed pass (single precision; the per-kind passes in double precision and under option 8) against one launch per seed -
    hit lists, bestJ, slot 0's result arrays."""
    s = trio[DEFAULT]
    seeds = np.concatenate([_leaf_seeds(s, 40 + rot), np.roll(s.crafted, rot)])
    _same_everywhere(trio, seeds)
    # slot 0 a crafted profile seed: its result arrays are the ones sweep_results reads
    _same_everywhere(trio, seeds[::-1].copy())


@pytest.mark.parametrize("rot", range(4))
def test_four_crafted_profile_seeds_alone(trio, rot):
    """0 + 4: k_sweep_nt_profq_multi in both precisions"""
    s = trio[DEFAULT]
    seeds = np.roll(s.crafted, rot)
    _same_everywhere(trio, seeds)
    s.ops.timer_start()
    _batch(s, seeds)
    s.ops.timer_stop_ms()
    assert s.ops.sweep_kernel_ms()[1] == 1 and s.ops.sweep_kernel_sweeps() == 4   # one launch stood for the four sweeps


def test_crafted_seeds_against_the_cpu_oracle(trio):
    """every crafted profile seed of a 4 + 4 batch against the reference restatement (tests/oracle.py): distance, weight and criterion
    of every active target, bit for bit."""
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
    seeds = np.concatenate([_leaf_seeds(s, 77), s.crafted])
    hits, best = _batch(s, seeds)
    for slot in range(4, 8):
        exp = orc.set_best_hit(ost, int(seeds[slot]), st.n_active, st.n_diff_allow, od, na)
        h = hits[slot]
        j = h["j"].astype(np.int64)
        assert np.array_equal(np.sort(j), s.active)
        assert np.array_equal(h["dist"], exp["dist"][j])
        assert np.array_equal(h["criterion"], exp["crit"][j])
        assert np.array_equal(h["weight"], exp["weight"][j])
        assert best[slot] == exp["best_j"]
