"""vft_ml_quartet_nni at `-mlacc 2` and `-mlacc 3`, operator level: the device's MLQuartetNNI (init -> {a workgroup per pairing ->
k_ml_nni_decide} x N -> verdict) against N rounds of the CPU oracle's MLQuartetOptimize per pairing, composed here the way MLQuartetNNI
(NJ.tcc:4885-5004) composes them at ml_accuracy >= 2: no alternative is ever dropped, the star-topology test (NJ.tcc:1688-1697) belongs to
AB|CD and is made again in every round.  With VFT_QUARTET_NO_STAR_TEST the composition is the oracle's quartet_optimize alone.

Quartets come from the final trees of thor_nt_150 (`-nt -mlacc 2`, Jukes-Cantor + CAT) and thor_aa_60_lg (`-lg -mlacc 2`): the splits with
the shortest internal branches, where the alternatives are contested and no star test fires, and as many with the longest, where it does.
Two of three quartets are handed over with B and C, or B and D, exchanged: the tree's split is then an alternative that has to win.
Every quartet owns five slots of branchlength[], so what the verdict writes there (DoNNI's assignment, NJ.tcc:5889-5915) is compared too.

Tolerances are those of the split-test mode of the same kernel (test_gpu_ml_lengths.py, test_quartet_likelihoods_against_the_reference):
optimised log-likelihoods 2e-5 relative in float32, lengths 1e-4 relative under Jukes-Cantor and 0.1 relative + 3e-4 under a matrix model
in float32.  A decision (star test, choice) is compared where the oracle's margin is wider than that tolerance on the two numbers it
compares; inside it either outcome is the reference's up to rounding, and the quartet's remaining numbers are compared only if the
decisions agree."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

import golden_util as G
from oracle import Oracle, tolerances

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ml_lengths as ML  # noqa: E402

pytestmark = pytest.mark.gpu

DT = np.float32
FTOL, ATOL = 0.001, 1.0e-4           # MLFTolBranchLength, MLMinBranchLengthTolerance (float32)
RTOL = 2e-5                          # optimised quartet log-likelihoods, float32
NO_STAR_TEST = 1                     # VFT_QUARTET_NO_STAR_TEST
SETS = {"thor_nt_150": 32, "thor_aa_60_lg": 16}   # fixture: quartets


class Result(C.Structure):
    _fields_ = [("criteria", C.c_double * 3), ("choice", C.c_int32), ("star", C.c_int32)]


def read_newick(text, n_leaves):
    """(child lists of the internal nodes, length per node, root): leaves s<i> are nodes i, internal nodes are numbered children first"""
    child, length, pos, nxt = {}, {}, [0], [n_leaves]
    leaf, blen = re.compile(r"s(\d+)"), re.compile(r":([0-9.eE+-]+)")

    def node():
        if text[pos[0]] == "(":
            kids = []
            while text[pos[0]] in "(,":
                pos[0] += 1
                kids.append(node())
            assert text[pos[0]] == ")"
            pos[0] += 1
            v = nxt[0]
            nxt[0] += 1
            child[v] = kids
        else:
            m = leaf.match(text, pos[0])
            v, pos[0] = int(m.group(1)), m.end()
        m = blen.match(text, pos[0])
        if m:
            length[v], pos[0] = float(m.group(1)), m.end()
        return v

    root = node()
    assert text[pos[0]] == ";" and root == nxt[0] - 1
    return child, length, root


@functools.lru_cache(maxsize=None)
def quartets(name):
    """The fixture's final tree as oracle profiles and the chosen quartets: dict of model tables, rates, tree arrays, per quartet the four
    oracle profiles, the ids of A, B, C, D (tree nodes; None: an up-profile to upload) and the five starting lengths."""
    from veryfasttree_amd import backend
    d = G.load(name)
    codes = d["codes"]
    n, n_pos = codes.shape
    n_codes = 4 if "_nt_" in name else 20
    assert len(backend.uniquify(codes)[0]) == n
    orc = Oracle(DT)
    min_len, min_rel, _ = tolerances(DT)
    tables = None if n_codes == 4 else backend.aa_model_tables("lg", DT)
    tm = None if tables is None else orc.tmat(*(tables[k] for k in ("stat", "statinv", "eigenval", "codefreq", "eigeninv", "eigeninvT")))
    rates, ratecat = d["r0_rates"], d["r0_ratecat"]
    child, length, root = read_newick(bytes(d["r0_newick"]).decode().strip(), n)
    assert len(child[root]) == 3 and all(len(child[v]) == 2 for v in child if v != root)
    bl = np.zeros(root + 1, DT)
    for v, x in length.items():
        bl[v] = x
    parent = {c: v for v, kids in child.items() for c in kids}
    post = lambda p, q, lp, lq: orc.posterior_profile(p, q, float(lp), float(lq), rates, ratecat, tm, min_len, min_rel)
    profs = {i: orc.leaf_profile(codes[i], n_codes) for i in range(n)}
    for v in range(n, root):
        a, b = child[v]
        profs[v] = post(profs[a], profs[b], bl[a], bl[b])
    ups = {}

    def up(p):
        """everything beyond p's branch, seen from p's parent (setupABCD's up-profile, NJ.tcc:1942-1975)"""
        if p not in ups:
            q = parent[p]
            others = [c for c in child[q] if c != p]
            if q == root:
                ups[p] = post(profs[others[0]], profs[others[1]], bl[others[0]], bl[others[1]])
            else:
                ups[p] = post(profs[others[0]], up(q), bl[others[0]], bl[q])
        return ups[p]

    inner = sorted(range(n, root), key=lambda v: (bl[v], v))
    count = SETS[name]
    qs = []
    for k, v in enumerate(inner[:count // 2] + inner[-(count // 2):]):
        a, b = child[v]
        p = parent[v]
        others = [c for c in child[p] if c != v]
        if p == root:
            c, dn, dlen, pd = others[0], others[1], others[1], profs[others[1]]
        else:
            c, dn, dlen, pd = others[0], None, p, up(p)
        ids, p4 = [a, b, c, dn], [profs[a], profs[b], profs[c], pd]
        lens = [float(bl[a]), float(bl[b]), float(bl[c]), float(bl[dlen]), float(bl[v])]
        # The tree is the end of a search: handed over as it stands, every quartet keeps AB|CD.  Two of three are handed over with B and
        # C, or B and D, exchanged, so that the split of the tree is the second or the third pairing and has to be found.
        swap = (None, 2, 3)[k % 3]
        if swap:
            for x in (ids, p4, lens):
                x[1], x[swap] = x[swap], x[1]
        qs.append(dict(node=v, ids=ids, profs=tuple(p4), lens=lens))
    return dict(d=d, orc=orc, n=n, n_pos=n_pos, n_codes=n_codes, tables=tables, tm=tm, rates=rates, ratecat=ratecat, child=child, root=root,
                bl=bl, quartets=qs)


def star_test(S, p4, lens):
    """the head of MLQuartetOptimize with pStarTest (NJ.tcc:1653-1697) on the oracle's operators:
    (fired, the value it returns when fired, the internal length, margin of the comparison)"""
    orc, min_len, min_rel = S["orc"], *tolerances(DT)[:2]
    args = (S["rates"], S["ratecat"], S["tm"])
    pa, pb, pc, pd = p4
    l = [max(x, min_len) for x in lens]
    ab = orc.posterior_profile(pa, pb, l[0], l[1], *args, min_len, min_rel)
    cd = orc.posterior_profile(pc, pd, l[2], l[3], *args, min_len, min_rel)
    vals = {}

    def f(x):
        vals[x] = -orc.pair_loglk(ab, cd, x, *args, min_rel)
        return vals[x]

    x = ML.min_branch_length(f, min_len, l[4], ML.MAX_BRANCH_LENGTH, FTOL, ATOL)
    best = -vals[x]
    star = -f(min_len)
    value = best + orc.pair_loglk(pa, pb, l[0] + l[1], *args, min_rel) + orc.pair_loglk(pc, pd, l[2] + l[3], *args, min_rel)
    return star < best - ML.CLOSE_LOGLK_LIMIT, value, x, (best - ML.CLOSE_LOGLK_LIMIT) - star


@functools.lru_cache(maxsize=None)
def expected(name, accuracy, star_on):
    """MLQuartetNNI at ml_accuracy >= 2 (NJ.tcc:4893-4982 without the branch of :4957) and DoNNI's lengths, per quartet:
    (criteria[3], choice, star, lengths A B C D I, the narrowest margin of a star test made, rounds run)"""
    assert accuracy >= 2
    S = quartets(name)
    orc, (min_len, min_rel, _) = S["orc"], tolerances(DT)
    out = []
    for q in S["quartets"]:
        pa, pb, pc, pd = q["profs"]
        A, B, Cl, D, I = q["lens"]
        pairing = [(pa, pb, pc, pd), (pa, pc, pb, pd), (pa, pd, pc, pb)]
        lens = [[A, B, Cl, D, I], [A, Cl, B, D, I], [A, D, Cl, B, I]]
        crit, star, margin = [0.0, 0.0, 0.0], False, np.inf
        for _ in range(accuracy):
            if star_on:
                star, value, x, m = star_test(S, pairing[0], lens[0])
                margin = min(margin, abs(m))
                if star:
                    crit = [value, -1e20, -1e20]
                    final = [A, B, Cl, D, x]
                    break
            for t in range(3):
                crit[t] = ML.quartet_optimize(orc, *pairing[t], lens[t], S["rates"], S["ratecat"], S["tm"], min_len, min_rel, FTOL, ATOL)
        choice = 0
        if not star:
            if crit[1] > crit[0] and crit[1] > crit[2]:
                choice = 1
            elif crit[2] > crit[0] and crit[2] > crit[1]:
                choice = 2
            L = lens[choice]
            final = [L[0], L[(1, 2, 3)[choice]], L[(2, 1, 2)[choice]], L[(3, 3, 1)[choice]], L[4]]
        out.append((list(crit), choice, star, final, margin))
    return out


@pytest.fixture(scope="module", params=list(SETS))
def device(request):
    """the quartets' profiles on the device: the tree's down-profiles computed there (bit-identical to the oracle's, test_gpu_ml_bits.py),
    the up-profiles uploaded into free internal slots, as test_quartet_likelihoods_against_the_reference does"""
    from veryfasttree_amd import HipProfileOps
    name = request.param
    S = quartets(name)
    n, root, child, bl, qs = S["n"], S["root"], S["child"], S["bl"], S["quartets"]
    ops = HipProfileOps(n, S["n_pos"], S["n_codes"], DT, max_nodes=3 * n + len(qs))
    ops.upload_leaves(S["d"]["codes"])
    ops.set_rates(S["rates"], S["ratecat"])
    ops.set_ml_limits(*tolerances(DT))
    if S["tables"] is not None:
        t = S["tables"]
        ops.set_transition_matrix(t["stat"], t["statinv"], t["eigenval"], t["codefreq"], t["eigeninv"], t["eigeninvT"])
    ops.set_max_node(ops.max_nodes)
    ops.branch_lengths_set(0, bl)
    level = {i: 0 for i in range(n)}
    for v in range(n, root):
        level[v] = 1 + max(level[c] for c in child[v])
    for lv in range(1, max(level.values()) + 1):   # recomputeMLProfiles
        batch = np.array([v for v in range(n, root) if level[v] == lv])
        c0, c1 = np.array([child[v][0] for v in batch]), np.array([child[v][1] for v in batch])
        ops.posteriorProfileBlen(batch, c0, c1, c0, c1)
    ops.synchronize()
    ids = np.zeros((len(qs), 4), np.int64)
    for k, q in enumerate(qs):
        ids[k] = [root + 1 + k if x is None else x for x in q["ids"]]
        if None in q["ids"]:
            ops.profile_upload(root + 1 + k, q["profs"][q["ids"].index(None)])
    assert ids.max() < ops.max_nodes
    li = np.arange(5 * len(qs), dtype=np.int64).reshape(-1, 5)      # quartet k owns slots 5k .. 5k+4 of branchlength[]
    assert li.max() < ops.max_nodes
    start = np.array([q["lens"] for q in qs], DT)

    def run(accuracy, star_on):
        from veryfasttree_amd.backend import _ptr
        ops.branch_lengths_set(0, start.reshape(-1))
        res = (Result * len(qs))()
        rc = ops.lib.vft_ml_quartet_nni_flags(ops.ctx, C.c_int64(len(qs)), _ptr(ids), _ptr(li), C.c_double(FTOL), C.c_double(ATOL),
                                              C.c_double(ML.CLOSE_LOGLK_LIMIT), C.c_int32(accuracy), C.c_int32(0 if star_on else NO_STAR_TEST), res)
        assert rc == 0
        lengths = ops.branch_lengths_get(0, 5 * len(qs)).astype(np.float64).reshape(-1, 5)
        return [(list(r.criteria), int(r.choice), bool(r.star), list(lengths[k])) for k, r in enumerate(res)]

    yield name, run
    ops.close()


@pytest.mark.parametrize("star_on", [True, False])
@pytest.mark.parametrize("accuracy", [2, 3])
def test_quartet_nni_rounds_match_the_oracle(device, accuracy, star_on):
    name, run = device
    want, got, base = expected(name, accuracy, star_on), run(accuracy, star_on), run(1, star_on)
    len_tol = dict(rtol=1e-4, atol=1e-7) if "_nt_" in name else dict(rtol=0.1, atol=3e-4)
    stars = moved = undecided = 0
    for k, ((wc, wchoice, wstar, wlen, margin), (gc, gchoice, gstar, glen)) in enumerate(zip(want, got)):
        tol = 2 * RTOL * abs(wc[0])
        rel = max(abs(g - w) / abs(w) for g, w in zip(gc, wc) if w > -1e19)
        print("%s acc %d star %d quartet %2d: oracle %s choice %d star %d | device %s choice %d star %d | rel %.2e, lengths off %.2e" % (
            name, accuracy, star_on, k, np.round(wc, 4), wchoice, wstar, np.round(gc, 4), gchoice, gstar, rel, np.abs(np.array(glen) - wlen).max()))
        if gstar != wstar:
            assert margin <= tol, (k, margin, tol)
            undecided += 1
            continue
        stars += wstar
        assert np.allclose(gc, wc, rtol=RTOL, atol=0), (k, gc, wc)
        if gchoice != wchoice:
            top = sorted(wc)
            assert top[2] - top[1] <= tol, (k, wc, gchoice)
            undecided += 1
            continue
        moved += wchoice != 0
        assert np.allclose(glen, wlen, **len_tol), (k, glen, wlen)
    print("%s acc %d star %d: %d star tests fired, %d quartets rearranged, %d decisions inside the tolerance" % (name, accuracy, star_on, stars, moved, undecided))
    # the test's own inputs: half of the quartets (the long internal branches) leave no decision to rounding, and every verdict occurs
    decisive = sum(1 for wc, _, wstar, _, margin in want
                   if margin > 2 * RTOL * abs(wc[0]) and (wstar or sorted(wc)[2] - sorted(wc)[1] > 2 * RTOL * abs(wc[0])))
    assert decisive >= len(want) // 2 and {w[1] for w in want} == {0, 1, 2}
    if star_on:
        assert 0 < stars < len(want)          # both ways out of the star test are taken
    else:
        assert stars == 0 and not any(g[2] for g in got)
    # the thorough rounds are not the default's: at accuracy 1 alternatives are dropped after the first round, here never
    differ = [k for k, (g, b) in enumerate(zip(got, base)) if g != b]
    print("%s acc %d star %d: %d of %d quartets differ from accuracy 1" % (name, accuracy, star_on, len(differ), len(got)))
    assert differ


def test_star_test_flag_only_matters_where_a_star_fires(device):
    """star test on against off at accuracy 2: a quartet whose star test never fires is the same computation, bit for bit; one whose
    test fires keeps AB|CD, reports -1e20 for the alternatives and moves the internal branch alone"""
    name, run = device
    on, off = run(2, True), run(2, False)
    start = np.array([q["lens"] for q in quartets(name)["quartets"]], DT).astype(np.float64)
    for k, (a, b) in enumerate(zip(on, off)):
        if not a[2]:
            assert a == b, k
        else:
            assert a[1] == 0 and a[0][1] == -1e20 and a[0][2] == -1e20
            assert a[3][:4] == list(start[k][:4])
