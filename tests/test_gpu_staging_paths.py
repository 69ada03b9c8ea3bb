"""Both transport paths of the calls that have two (veryfasttree_amd/csrc/vft_staging.h, Stage in vft_api.hip): a list that fits its
site's ring limit travels through the host-mapped ring, a longer one through the device scratch.  Each call runs at the longest list
that still takes the ring and at one element more, and must give - bit for bit - what the same list gives when it is issued in chunks
of 1 000, the short-list path that test_gpu_parity.py and test_gpu_ml_bits.py pin against the reference's goldens and the oracle.
Same kernels, same inputs: the tolerance is equality.

    vft_average_profiles          4 x pad256(8 n) <= 256 KiB     n =  8 192 | 8 193
    vft_posterior_profiles        5 x 8 n <= 512 KiB             n = 13 107 | 13 108   (tile streams, and dense rows)
    vft_posterior_profiles_blen   7 x 8 n <= 256 KiB             n =  4 681 | 4 682
    vft_pair_loglk                4 x 8 n <= 512 KiB             n = 16 384 | 16 385
    vft_pair_distances            2 ids + 3 results + stale ids + wait indices, each padded to 256 bytes, <= 256 KiB:
                                  n = 7 264 (f32) / 5 440 (f64) with nothing stale, fewer with every leaf stale
    vft_block_distances           8 (nA + nB + nStale) <= 256 KiB   nA + nB = 32 768 | 32 769

The smallest shape that works: 300 nucleotide leaves x 64 columns (one column chunk of 16 would do for the kernels; 64 is four), float32
and float64, and room for two sets of 13 108 internal nodes - the calls that write nodes name n + 1 distinct outputs, once for the whole
list and once for the chunks.  Written nodes are compared on the device (vft_profiles_differ: bit-identical or not, which
test_gpu_chains.py checks against downloads), and a few of them, the chunk seams among them, are downloaded and compared element for element.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64, I32, P = C.c_int64, C.c_int32, C.c_void_p
N_LEAVES, N_POS, CHUNK, RING = 300, 64, 1000, 256 << 10
N_OUT = 13108
X0, Y0 = N_LEAVES, N_LEAVES + N_OUT   # outputs of the whole list / of the chunks
MAX_NODES = N_LEAVES + 2 * N_OUT
N_ACTIVE, N_DIFF_ALLOW = N_LEAVES, 3
DTYPES = [np.float32, np.float64]
SIDES = [0, 1]   # the boundary itself (ring) and one more (scratch)


def pad(b):
    return (b + 255) // 256 * 256


def pair_boundary(rs, n_stale):
    n = 1
    while 2 * pad(8 * (n + 1)) + 3 * pad(rs * (n + 1)) + pad(8 * n_stale) + pad(8 * (n + 1)) <= RING:
        n += 1
    return n


def make(dt, rows):
    from veryfasttree_amd import HipProfileOps, synth
    codes = synth.random_descent_codes(N_LEAVES, N_POS, 4, 0.05, 0.03, seed=11)
    ops = HipProfileOps(N_LEAVES, N_POS, 4, dt, max_nodes=MAX_NODES)
    ops.upload_leaves(codes)
    z = np.zeros(N_LEAVES, dt)
    ops.set_node_scalars(0, z, (codes != 127).sum(1).astype(dt), z)
    ops.outProfile(np.arange(N_LEAVES))
    ops.set_out_distances(0, z, np.full(N_LEAVES, 10 * N_LEAVES))
    ops.setOutDistance(None, N_ACTIVE, 0.0)
    ops.set_max_node(MAX_NODES)
    if rows:   # the ML stage's layout: every internal profile a dense row, lengths on the device
        ops.set_profile_rows(True)
        ops.branch_lengths_set(0, np.random.default_rng(3).uniform(0.001, 0.4, MAX_NODES).astype(dt))
    return ops


@pytest.fixture(scope="module", params=DTYPES, ids=["f32", "f64"])
def nj(request):
    ops = make(request.param, False)
    yield ops
    ops.close()


@pytest.fixture(scope="module", params=DTYPES, ids=["f32", "f64"])
def ml(request):
    ops = make(request.param, True)
    yield ops
    ops.close()


def chunks(n):
    return [(k, min(k + CHUNK, n)) for k in range(0, n, CHUNK)]


def children(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, N_LEAVES, n).astype(np.int64)
    b = (a + rng.integers(1, N_LEAVES, n)) % N_LEAVES   # never a itself
    return rng, a, b


def same(p, q):
    (w1, c1, f1), (w2, c2, f2) = p, q
    vec = (w1 > 0) & (c1 == 127)
    return np.array_equal(w1.view(np.uint8), w2.view(np.uint8)) and np.array_equal(c1, c2) and np.array_equal(f1[vec].view(np.uint8), f2[vec].view(np.uint8))


def assert_written_nodes_equal(ops, n):
    x, y = np.arange(X0, X0 + n, dtype=np.int64), np.arange(Y0, Y0 + n, dtype=np.int64)
    differ = np.ones(n, np.int32)
    for k in range(0, n, 4096):
        m = min(4096, n - k)
        assert ops.lib.vft_profiles_differ(ops.ctx, I64(m), x[k:k + m].ctypes.data_as(P), y[k:k + m].ctypes.data_as(P), differ[k:k + m].ctypes.data_as(P)) == 0
    assert not differ.any(), np.flatnonzero(differ)[:10]
    for k in (0, CHUNK - 1, CHUNK, n - CHUNK, n - 2, n - 1):   # the seams of the chunks and both ends, element for element
        assert same(ops.profile_download(int(x[k])), ops.profile_download(int(y[k]))), k
    # (and the comparison sees a difference where there is one: neighbours have other children)
    m = 64
    assert ops.lib.vft_profiles_differ(ops.ctx, I64(m), x[:m].ctypes.data_as(P), y[1:m + 1].ctypes.data_as(P), differ[:m].ctypes.data_as(P)) == 0
    assert differ[:m].any()


@pytest.mark.parametrize("side", SIDES)
def test_average_profiles(nj, side):
    n = 8192 + side
    _, a, b = children(n, 21)
    nj.averageProfile(np.arange(X0, X0 + n), a, b)
    for lo, hi in chunks(n):
        nj.averageProfile(np.arange(Y0 + lo, Y0 + hi), a[lo:hi], b[lo:hi])
    assert_written_nodes_equal(nj, n)


def posterior_profiles(ops, side):
    n = 13107 + side
    rng, a, b = children(n, 22)
    l1, l2 = rng.uniform(0.001, 0.5, n), rng.uniform(0.001, 0.5, n)
    ops.posteriorProfile(np.arange(X0, X0 + n), a, b, l1, l2)
    for lo, hi in chunks(n):
        ops.posteriorProfile(np.arange(Y0 + lo, Y0 + hi), a[lo:hi], b[lo:hi], l1[lo:hi], l2[lo:hi])
    assert_written_nodes_equal(ops, n)


@pytest.mark.parametrize("side", SIDES)
def test_posterior_profiles_into_tile_streams(nj, side):
    posterior_profiles(nj, side)


@pytest.mark.parametrize("side", SIDES)
def test_posterior_profiles_into_rows(ml, side):
    posterior_profiles(ml, side)


@pytest.mark.parametrize("side", SIDES)
def test_posterior_profiles_blen(ml, side):
    n = 4681 + side
    rng, a, b = children(n, 23)
    la, lb = rng.integers(0, MAX_NODES, n).astype(np.int64), rng.integers(0, MAX_NODES, n).astype(np.int64)
    ml.posteriorProfileBlen(np.arange(X0, X0 + n), a, b, la, lb)
    for lo, hi in chunks(n):
        ml.posteriorProfileBlen(np.arange(Y0 + lo, Y0 + hi), a[lo:hi], b[lo:hi], la[lo:hi], lb[lo:hi])
    assert_written_nodes_equal(ml, n)


@pytest.mark.parametrize("side", SIDES)
def test_pair_loglk(nj, side):
    n = 16384 + side
    rng, a, b = children(n, 24)
    length = rng.uniform(0.001, 0.5, n)
    whole = nj.pairLogLk(a, b, length)
    parts = np.concatenate([nj.pairLogLk(a[lo:hi], b[lo:hi], length[lo:hi]) for lo, hi in chunks(n)])
    assert np.all(np.isfinite(whole)) and len(np.unique(whole)) > n // 2
    assert np.array_equal(whole.view(np.uint8), parts.view(np.uint8))


@pytest.mark.parametrize("stale", [False, True], ids=["fresh", "stale"])
@pytest.mark.parametrize("side", SIDES)
def test_pair_distances(nj, side, stale):
    rs = nj.dt.itemsize
    n = pair_boundary(rs, N_LEAVES if stale else 0) + side
    assert pair_boundary(4, 0) == 7264 and pair_boundary(8, 0) == 5440
    _, i, j = children(n, 25)
    assert not stale or len(np.unique(np.concatenate([i, j]))) == N_LEAVES   # every leaf is named: nStale is N_LEAVES

    def spoil():   # every leaf's out-distance wrong and stamped long ago: the lists refresh what they name
        if stale:
            nj.set_out_distances(0, np.full(N_LEAVES, 1e3, nj.dt), np.full(N_LEAVES, 10 * N_LEAVES))

    spoil()
    whole = nj.setDistCriterion(i, j, N_ACTIVE, N_DIFF_ALLOW, 0.0)
    spoil()
    parts = [nj.setDistCriterion(i[lo:hi], j[lo:hi], N_ACTIVE, N_DIFF_ALLOW, 0.0) for lo, hi in chunks(n)]
    for k in range(3):
        got, want = whole[k], np.concatenate([p[k] for p in parts])
        assert np.all(np.isfinite(got)) and len(np.unique(got)) > (1 if k == 1 else 100)   # (weights count columns: a dozen values)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), k


@pytest.mark.parametrize("side", SIDES)
def test_block_distances(nj, side):
    n_b = 32768 - 2 + side
    rng = np.random.default_rng(26)
    a = np.array([5, 250], np.int64)
    b = rng.integers(0, N_LEAVES, n_b).astype(np.int64)
    whole = nj.blockDistances(a, b, N_ACTIVE, N_DIFF_ALLOW, 0.0)
    parts = np.concatenate([nj.blockDistances(a, b[lo:hi], N_ACTIVE, N_DIFF_ALLOW, 0.0) for lo, hi in chunks(n_b)], axis=1)
    ok = b[None, :] != a[:, None]   # (slots of i == j are unspecified)
    assert np.all(np.isfinite(whole[ok])) and len(np.unique(whole[ok])) > 100
    assert np.array_equal(whole[ok].view(np.uint8), parts[ok].view(np.uint8))
