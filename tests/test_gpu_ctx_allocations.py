"""Every device and pinned-host allocation of a context belongs to one owner (veryfasttree_amd/csrc/vft_owned.h), sweep slot 0 is a
slot like the others, and vft_allocation_count reads the owner: subsystems that are created and destroyed give their allocations
back, buffers that are reused or regrown keep the count, a refused creation leaves it alone, and a context can be made, used and
destroyed over and over.  (What happens when an allocation FAILS is the CPU program's business: tests/test_owned_cpu.py.)

The smallest shapes at which the paths differ - mid-NJ states of veryfasttree_amd.workload.TopHitsState, as in test_gpu_mixed_pass.py:

    nt_f32   130 sequences x 70 columns, float32, max_nodes = 3 n: three leaf tiles (the last partial), five 16-column chunks (the
             last partial); sweep slots beyond 0 carry staged-query buffers
    aa_f64   70 sequences x 33 columns, float64, with the BLOSUM45 distance matrix: slots without staged-query buffers, and the
             query's piece table (qPT) is real

"The count" is always taken after a first, warm-up use of the call under test: buffers that OTHER calls make on first use must not
look like growth.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {"nt_f32": (130, 70, 4, np.float32, 40, 41), "aa_f64": (70, 33, 20, np.float64, 20, 42)}
N_SEEDS = 8


class _State:
    pass


def _context(shape):
    from veryfasttree_amd import HipProfileOps, backend, synth
    n, L, nc, dt, _, seed = SHAPES[shape]
    codes = synth.random_descent_codes(n, L, nc, 0.05, 0.1, seed=seed)
    ops = HipProfileOps(n, L, nc, dt, max_nodes=3 * n)
    if nc == 20:
        t = backend.distance_tables(None, dt)
        ops.set_distance_matrix(t["distances"], t["codefreq"], t["eigenval"], t["eigentot"])
    return ops, codes


def _make(shape):
    from veryfasttree_amd.workload import TopHitsState
    n, n_join, seed = SHAPES[shape][0], SHAPES[shape][4], SHAPES[shape][5]
    ops, codes = _context(shape)
    s = _State()
    s.ops, s.st, s.n = ops, TopHitsState(ops, codes, n_join), n
    s.k = s.st.n_active
    # four leaf seeds and four profile seeds: in single precision on nucleotides the batch is one mixed pass
    rng = np.random.default_rng(seed)
    act = s.st.active
    s.seeds = np.concatenate([rng.choice(act[act < n], N_SEEDS // 2, replace=False), rng.choice(act[act >= n], N_SEEDS // 2, replace=False)])
    rng.shuffle(s.seeds)
    return s


def _batch(s):
    st = s.st
    return s.ops.setBestHitBatch(s.seeds, st.n_active, st.n_diff_allow, st.totdiam, s.k)


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request):
    s = _make(request.param)
    yield s
    s.ops.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exhaustive_matrix_gives_its_allocations_back(shape):
    o, codes = _context(shape)   # (the matrix wants unjoined leaves: a context with nothing but the leaves)
    o.upload_leaves(codes)
    o.exhaustive_create()
    o.exhaustive_fill()
    assert o.lib.vft_exhaustive_destroy(o.ctx) == 0   # warm-up: what the fill makes on first use exists from here on
    before = o.allocation_count()
    counts = []
    for _ in range(2):
        o.exhaustive_create()
        o.exhaustive_fill()
        counts.append(o.allocation_count())
        assert counts[-1][0] == before[0] + 6 and counts[-1][1] > before[1]
        assert o.lib.vft_exhaustive_destroy(o.ctx) == 0
        assert o.allocation_count() == before
        assert o.lib.vft_exhaustive_destroy(o.ctx) == 0   # callable any time
        assert o.allocation_count() == before
    assert counts[0] == counts[1]
    o.close()


def test_a_second_batch_reuses_the_slots_and_slot_0_is_the_single_sweeps(state):
    s = state
    hits1, best1 = _batch(s)
    after_first = s.ops.allocation_count()
    hits2, best2 = _batch(s)
    assert s.ops.allocation_count() == after_first
    assert np.array_equal(hits1, hits2) and np.array_equal(best1, best2)
    st = s.st
    one, best = s.ops.setBestHit(int(s.seeds[0]), st.n_active, st.n_diff_allow, st.totdiam, s.k)
    assert np.array_equal(one, hits1[0]) and best == best1[0]
    assert s.ops.allocation_count() == after_first
    # every active target is in every list (k = their number)
    for h in hits1:
        assert np.array_equal(np.sort(h["j"]), st.active)


def test_growing_pair_lists_regrow_the_scratch_in_place(state):
    s = state
    st = s.st
    rng = np.random.default_rng(5)
    seen = []
    # Beyond 256 KiB of ids and results a list goes through the scratch buffer: 2 ids and 3 results per pair, and a buffer that is too
    # small is replaced by one half as large again as the request.  The scratch the state's builder left is no larger than everything
    # the context owns, so the first list (the warm-up) outgrows it, and each later list is twice the one before: two more regrows.
    per_pair = 16 + 3 * s.ops.dt.itemsize
    first = s.ops.allocation_count()[1] // per_pair + 1
    for n_pairs in (first, 2 * first, 4 * first):
        assert n_pairs * per_pair > 256 << 10   # not through the small-list ring
        i = rng.choice(st.active, n_pairs)
        j = rng.choice(st.active, n_pairs)
        j[i == j] = st.active[0]
        i[i == j] = st.active[1]
        d, w, c = s.ops.setDistCriterion(i, j, st.n_active, st.n_diff_allow, st.totdiam)
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(c))
        seen.append(s.ops.allocation_count())
    assert seen[0][0] == seen[1][0] == seen[2][0]
    assert seen[0][1] < seen[1][1] < seen[2][1]


def test_refused_creations_leave_the_count_alone(state):
    import ctypes as C
    from veryfasttree_amd import VftError
    from veryfasttree_amd.backend import I32, I64
    ops = state.ops
    ops.tophits_create(16)
    count = ops.allocation_count()
    with pytest.raises(VftError, match="vft_tophits_create: lists exist already"):
        ops.tophits_create(16)
    assert ops.lib.vft_tophits_create(ops.ctx, I32(16), I64(ops.max_nodes)) == 3   # VFT_ERR_STATE
    assert ops.allocation_count() == count

    class Cfg(C.Structure):   # vft_nj_engine_config
        _fields_ = [("m", I32), ("n_top", I32), ("need", I32), ("age_limit", I32), ("fastest", I32), ("pad", I32), ("stale_stamp", I64),
                    ("stale_out_limit", C.c_double)]
    cfg = Cfg(8, 12, 4, 10, 0, 0, 10 * state.n, 0.01)   # m = 8: not the lists' 16
    assert ops.lib.vft_nj_engine_create(ops.ctx, C.byref(cfg)) == 3
    assert ops.lib.vft_last_error(ops.ctx).decode() == "vft_nj_engine_create: vft_tophits_create(m) first"
    assert ops.allocation_count() == count


@pytest.mark.parametrize("shape", list(SHAPES))
def test_create_use_destroy_cycles(shape):
    runs = []
    for _ in range(3):
        s = _make(shape)
        runs.append(_batch(s))
        assert s.ops.allocation_count()[0] > 0
        assert s.ops.lib.vft_destroy(s.ops.ctx) == 0
        s.ops.ctx = None
    for hits, best in runs[1:]:
        assert np.array_equal(hits, runs[0][0]) and np.array_equal(best, runs[0][1])
