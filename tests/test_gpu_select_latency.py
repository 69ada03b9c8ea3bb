"""GPU: the top-k selection (k_select_hist / k_select_collect / k_select_rank) against an independent reference, at the shapes where its
loads can go wrong: criteria read as 16-byte vectors with scalar edges, a thread's share issued in unrolled batches, the (min, max)
pairs of the sweep read as vectors with a scalar tail, the best join found with ballots among the first 64 records.

The reference is numpy on the sweep's own result arrays (slot 0, `sweep_results`): criterion ascending, id descending, sentinels
(>= 1e20) out, cut at k, empty records behind; bestJ = the smallest id among the minimal criteria, the query excluded.  Seeds in other
slots of a batch are compared with their own single `setBestHit`.

The constants the shapes are built around (vft_kernels_nj.h):"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEL_WGS, WG = 128, 256          # VFT_SEL_WGS workgroups of VFT_WG threads
SEL_BATCH = 10                  # VFT_SEL_BATCH vectors per thread and batch
PART_BATCH = 5                  # VFT_SEL_PART_BATCH vectors of (min, max) pairs per thread and batch
RANK_TILE = 2048                # VFT_RANK_TILE


def vec(dt):
    return 16 // np.dtype(dt).itemsize


def reference(ops, maxnode, query, k, lo, hi):
    dist, weight, crit = ops.sweep_results(0, maxnode)
    ids = np.arange(lo, min(hi, maxnode), dtype=np.int64)
    ids = ids[crit[ids] < 1e20]
    order = ids[np.lexsort((-ids, crit[ids]))]
    others = order[order != query]
    best = -1
    if len(others):
        best = int(others[crit[others] == crit[others[0]]].min())
    run = int((crit[order] == crit[order[0]]).sum()) if len(order) else 0
    exp = np.zeros(k, ops.hit_dtype)
    exp["j"], exp["dist"], exp["criterion"] = -1, 1e20, 1e20
    top = order[:k]
    exp["j"][:len(top)] = top
    exp["dist"][:len(top)] = dist[top]
    exp["weight"][:len(top)] = weight[top]
    exp["criterion"][:len(top)] = crit[top]
    cut_tie = len(order) > k and crit[order[k - 1]] == crit[order[k]]
    return exp, best, run, cut_tie


def check(ops, st, q, k, lo=0, hi=None):
    hi = st.maxnode if hi is None else hi
    hits, best = ops.setBestHit(int(q), st.n_active, st.n_diff_allow, st.totdiam, k, want_best=k >= 2)
    exp, ebest, run, cut_tie = reference(ops, st.maxnode, int(q), k, lo, hi)
    assert np.array_equal(hits, exp), "records differ (query %d, k %d, ids [%d, %d))" % (q, k, lo, hi)
    if k >= 2:   # (the API returns no best join below two records)
        assert best == ebest, "bestJ %d, expected %d (query %d, k %d, ids [%d, %d), run %d)" % (best, ebest, q, k, lo, hi, run)
    return hits, best, run, cut_tie


def make_state(n, L, n_codes, dt, n_join, p=0.05, seed=5, codes=None):
    from veryfasttree_amd import HipProfileOps, synth
    from veryfasttree_amd.workload import TopHitsState
    if codes is None:
        codes = synth.random_descent_codes(n, L, n_codes, p, 0.02, seed=seed)
    ops = HipProfileOps(n, L, n_codes, dt)
    if n_codes == 20:
        import golden_util as G
        dm = G.load("wb_aa_f32")
        ops.set_distance_matrix(dm["dmat.distances"], dm["dmat.codefreq"], dm["dmat.eigenval"], dm["dmat.eigentot"])
    return ops, TopHitsState(ops, codes, n_join)


@pytest.mark.parametrize("n_codes,dt", [(4, np.float32), (4, np.float64), (20, np.float32)])
def test_vector_head_and_tail(n_codes, dt):
    """Spans of 1 .. 5 ids (every residue of hi mod 4, fewer ids than one vector), 255 / 256 / 257 (one workgroup's first round), with lo 0
    and 64; 1 400 and 1 500 ids: a leaf seed's sweep leaves ceil(span / 256) = 6 (min, max) pairs - one vector of floats and a tail of
    two, three vectors of doubles - a profile seed's another count."""
    n = 1600
    ops, st = make_state(n, 16, n_codes, dt, 20)   # (ids 0 .. 39 are joined: the short spans at lo = 0 hold sentinels only)
    leaf = int(st.active[st.active < n][3])
    prof = int(st.active[st.active >= n][5])
    for lo in (0, 64):
        for span in (1, 2, 3, 4, 5, 255, 256, 257, 1400, 1500):
            ops.set_shard(lo, lo + span)
            check(ops, st, leaf, 8, lo, lo + span)
    for span in (1, 3, 257, 1400, st.maxnode - 64):
        ops.set_shard(64, 64 + span)
        check(ops, st, prof, 8, 64, 64 + span)
    ops.set_shard(0, st.maxnode)
    check(ops, st, leaf, 40)
    check(ops, st, prof, 40)
    ops.close()


@pytest.fixture(scope="module")
def wide():
    """1 320 000 leaves of 16 columns: more ids than one unrolled batch of the whole grid takes (16 columns and not 8: few equal
    sequences, so that no 8 192 criteria tie at the k-th)."""
    n = 1320000
    ops, st = make_state(n, 16, 4, np.float32, 1000, p=0.3, seed=9)
    yield ops, st, int(st.active[st.active < n][11])
    ops.close()


GRID_PASS = SEL_WGS * WG * vec(np.float32)      # 131 072 ids: one vector per thread
ONE_BATCH = SEL_BATCH * GRID_PASS               # 1 310 720 ids: one unrolled batch per thread
PART_PASS = PART_BATCH * WG * vec(np.float32)   # 5 120 pairs = 1 310 720 ids of a leaf seed's sweep: one batch of (min, max) vectors


@pytest.mark.parametrize("span", [GRID_PASS - 1, GRID_PASS, GRID_PASS + 1, ONE_BATCH - 1, ONE_BATCH, ONE_BATCH + 1,
                                  ONE_BATCH + 17 * WG + 2])
def test_grid_pass_and_batch_boundaries(wide, span):
    """One id short of, exactly, and one id over: one pass of the grid with a vector per thread; one unrolled batch (the second batch then
    has a single scalar id, or one vector and none).  At ONE_BATCH the (min, max) pairs are exactly one batch of vectors too, one id
    more leaves one pair in the scalar tail, 17 workgroups more a second batch of pair vectors with a tail of two."""
    ops, st, q = wide
    assert span <= st.maxnode and PART_PASS * WG == ONE_BATCH
    ops.set_shard(0, span)
    check(ops, st, q, 50, 0, span)
    ops.set_shard(64, 64 + span)
    check(ops, st, q, 2, 64, 64 + span)
    ops.set_shard(0, st.maxnode)


def test_rank_sort_sizes():
    """k = 1 and 2; more records asked for than there are targets (empty records behind); 3 000 of 5 000: two tiles of the rank sort."""
    n = 5000
    ops, st = make_state(n, 16, 4, np.float32, 300, p=0.2, seed=2)
    q = int(st.active[st.active < n][7])
    p = int(st.active[st.active >= n][2])
    assert 3000 > RANK_TILE
    for k in (1, 2, 3000):
        check(ops, st, q, k)
        check(ops, st, p, k)
    ops.set_shard(0, 640)
    hits, _, _, _ = check(ops, st, q, 2000, 0, 640)
    assert (hits["j"] < 0).sum() >= 2000 - 640
    ops.set_shard(0, st.maxnode)
    ops.close()


GROUPS = (1, 2, 3, 63, 64, 65, 66, 67)   # identical sequences: runs of equal criteria around the 64 records wavefront 0 holds


@pytest.fixture(scope="module")
def tied():
    """Groups of identical sequences among random ones (no two of a group are joined: the joins take the first 40 leaves).  The members of
    a group have the same distance to anything and the same out-distance: the same criterion, bit for bit."""
    from veryfasttree_amd import synth
    n, L = 640, 64
    codes = synth.random_descent_codes(n, L, 4, 0.3, 0.0, seed=21)
    at, members = 100, []
    for g in GROUPS:
        codes[at:at + g] = codes[at]
        members.append(np.arange(at, at + g))
        at += g
    ops, st = make_state(n, L, 4, np.float32, 20, codes=codes)
    yield ops, st, members
    ops.close()


def test_runs_of_minimal_criteria(tied):
    """The seed is a member of a group of g identical sequences: the others tie at the minimum, dist 0 - a run of g - 1 records, or g
    where the seed's own record ties with them.  With the group sizes above the runs cover 1, 2, 63, 64 and 65 records either way: the
    ballot path, a run that ends exactly at record 64, and the serial scan behind it."""
    ops, st, members = tied
    runs = set()
    for m in members:
        q = int(m[len(m) // 2])   # (not the smallest id of its group: the best join is another member)
        _, best, run, _ = check(ops, st, q, 200)
        runs.add(run)
        if len(m) > 1:
            assert best == int(m[0]) or (q == int(m[0]) and best == int(m[1]))
    assert {1, 2, 63, 64, 65} <= runs | {r - 1 for r in runs}, "runs seen: %s" % sorted(runs)


def test_ties_across_the_cut_and_truncated_ties(tied):
    """The cut at k inside a group of equal criteria (id descending decides who stays); every one of the k records tied at the minimum -
    the list ends inside the run, and the best join is found among the criteria themselves; the seed among the minimal ones."""
    ops, st, members = tied
    big = members[-1]            # 67 identical sequences
    q = int(big[30])
    cut = 0
    for k in (2, 5, 40, 63, 64, 65, 66, 67, 70, 131, 200):
        _, best, run, cut_tie = check(ops, st, q, k)
        cut += bool(cut_tie)
        if k <= run - 1:         # truncated: ids below the cut tie as well, the smallest of the group wins
            assert best == int(big[0])
    assert cut >= 3, "no k cut a group of equal criteria"
    q0 = int(big[0])             # the seed is the smallest id of the run: the best join is the next one
    _, best, _, _ = check(ops, st, q0, 10)
    assert best == int(big[1])


def test_batches_of_1_8_and_9_seeds(tied):
    """Slot 0 against the numpy reference, the other slots against their own single selection; once with the candidate buffers poisoned."""
    ops, st, members = tied
    leaves, profs = st.active[st.active < st.n_seqs], st.active[st.active >= st.n_seqs]
    pool = np.concatenate([[int(members[-1][5]), int(profs[0]), int(members[3][9])], leaves[50:53], profs[3:6]]).astype(np.int64)
    k = 100
    single = [ops.setBestHit(int(q), st.n_active, st.n_diff_allow, st.totdiam, k) for q in pool]
    for count, poison in ((1, False), (8, False), (9, False), (8, True)):
        seeds = pool[:count]
        if poison:
            ops.debug_option(14, 1)   # VFT_DEBUG_POISON_SELECTION
        hits, best = ops.setBestHitBatch(seeds, st.n_active, st.n_diff_allow, st.totdiam, k)
        exp, ebest, _, _ = reference(ops, st.maxnode, int(seeds[0]), k, 0, st.maxnode)
        assert np.array_equal(hits[0], exp) and best[0] == ebest
        for s in range(count):
            assert np.array_equal(hits[s], single[s][0]) and best[s] == single[s][1], "seed %d of %d" % (s, count)
