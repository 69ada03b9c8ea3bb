"""One posteriorProfile under a 20-state matrix model (NJ.tcc:2335-2429) restated in numpy, rounding for rounding what the reference and
the device do: numeric_t products and the four strided accumulators of the SSE / AVX kernels ((s0 + s1) + (s2 + s3), vft_red4_*), the
P(t) table through libm's exp, double where the reference has double.  With `near` (nearP, nearFreq) the `-approxml` branch of
NJ.tcc:2390-2421 is taken where it holds; without it the result is tests/oracle.py's posterior_profile bit for bit
(tests/test_approxml_cpu.py anchors that before anything is compared with the device).

Also near_tables(): TransitionMatrix.tcc:227-279 restated, for the tables themselves."""
import math

import numpy as np

NOCODE = 127
MINF, MINRATIO, NEAR_T = 0.95, 2 / 3.0, 0.2     # Constants.h:46-49
# what became of a column: gap with gap / no state reached MINF / the ratio test gave up / the near-constant branch
GAP, NEVER, GAVE_UP, ROUGH = 0, 1, 2, 3


def red4_rows(v, M):
    """vft_red4_mul(v, M[j]) for every row j of M [rows, 20], in v's dtype"""
    s = np.zeros((M.shape[0], 4), v.dtype)
    for i in range(0, 20, 4):
        s = (v[i:i + 4] * M[:, i:i + 4]) + s     # p = a * b (rounded); s = p + s (rounded)
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def red4_sum(v):
    s = np.zeros(4, v.dtype)
    for i in range(0, 20, 4):
        s = v[i:i + 4] + s
    return (s[0] + s[1]) + (s[2] + s[3])


def exp_eigen_rates(length, rates, eigenval, min_rel):
    dt = eigenval.dtype.type
    out = np.zeros((len(rates), 20), eigenval.dtype)
    for r in range(len(rates)):
        rel = max(length * float(rates[r]), min_rel)
        x = eigenval * dt(rel)                    # numeric_t product
        out[r] = [dt(math.exp(float(v))) for v in x]
    return out


def posterior(p1, p2, len1, len2, rates, ratecat, tm, near=None, min_len=5e-4, min_rel=2.5e-4):
    """p1, p2: (w, c, f) with f in the model's eigen-space; tm: dict of stat, statinv, eigenval, codefreq [21, 20], eigeninv; near: None
    (exact ML) or (nearP, nearFreq).  Returns (w, c, f), what[n_pos] (GAP / NEVER / GAVE_UP / ROUGH), ch[n_pos] (the dominant state or
    -1) and fail[n_pos] (the first state whose ratio test failed, or -1)."""
    dtype = np.asarray(p1[0]).dtype
    dt = dtype.type
    t = {k: np.ascontiguousarray(v, dtype) for k, v in tm.items()}
    cf, statinv, eigeninv = t["codefreq"].reshape(21, 20), t["statinv"], t["eigeninv"].reshape(20, 20)
    rates = np.ascontiguousarray(rates, dtype)
    ee1 = exp_eigen_rates(max(len1, min_len), rates, t["eigenval"], min_rel)
    ee2 = exp_eigen_rates(max(len2, min_len), rates, t["eigenval"], min_rel)
    n_pos = len(p1[0])
    wo, co, fo = np.ones(n_pos, dtype), np.full(n_pos, NOCODE, np.uint8), np.zeros((n_pos, 20), dtype)
    what, chs, fails = np.zeros(n_pos, np.int64), np.full(n_pos, -1, np.int64), np.full(n_pos, -1, np.int64)

    def freq(p, i):
        w, c, f = p[0][i], int(p[1][i]), p[2][i]
        if w > 0 and c == NOCODE:
            return np.ascontiguousarray(f, dtype)
        v = cf[20 if c == NOCODE else c]
        wd = float(w)
        if 0.0 < wd < 1.0:                        # double arithmetic, stored as numeric_t
            v = (wd * v.astype(np.float64) + (1.0 - wd) * cf[20].astype(np.float64)).astype(dtype)
        return v

    for i in range(n_pos):
        if p1[1][i] == NOCODE and p2[1][i] == NOCODE and p1[0][i] == 0 and p2[0][i] == 0:
            wo[i] = 0
            continue
        r = int(ratecat[i])
        fm1, fm2 = freq(p1, i) * ee1[r], freq(p2, i) * ee2[r]
        value = (red4_rows(fm1, cf[:20]) * red4_rows(fm2, cf[:20])) * statinv
        fpost = np.where(value >= 0, value, dt(0))
        fpost = fpost * dt(1.0 / float(red4_sum(fpost)))
        what[i] = NEVER
        ch, w = -1, 0.0
        if near is not None:
            near_p, near_freq = (np.ascontiguousarray(x, dtype).reshape(20, 20) for x in near)
            for j in range(20):
                if float(fpost[j]) >= MINF:
                    ch = j
                    break
            chs[i] = ch
            if ch >= 0:
                w = float(fpost[ch] - near_p[ch, ch]) / (1.0 - float(near_p[ch, ch]))   # numeric_t - numeric_t, then double
                for j in range(20):
                    if j != ch and (1.0 - w) * float(near_p[ch, j]) < float(fpost[j]) * MINRATIO:
                        fails[i] = j
                        what[i] = GAVE_UP
                        ch = -1
                        break
        if ch >= 0:
            what[i] = ROUGH
            w_inv_stat = w * float(statinv[ch])
            fo[i] = [dt(w_inv_stat * float(cf[ch, j]) + (1.0 - w) * float(near_freq[ch, j])) for j in range(20)]
        else:
            fo[i] = red4_rows(fpost, eigeninv)
    return (wo, co, fo), what, chs, fails


def near_tables(stat, eigenval, codefreq, eigeninv):
    """TransitionMatrix.tcc:227-279 from the stored (numeric_t) tables: double arithmetic in the reference's order, libm's exp; the result
    narrowed to the tables' dtype.  (The rotation's inner product reads codeFreq[i][j] for every k - as the reference's does.)"""
    dtype = np.asarray(stat).dtype
    stat, eigenval = [float(x) for x in stat], [float(x) for x in eigenval]
    cf = [[float(x) for x in row] for row in np.asarray(codefreq).reshape(21, 20)]
    ei = [[float(x) for x in row] for row in np.asarray(eigeninv).reshape(20, 20)]
    expv = [math.exp(NEAR_T * eigenval[i]) for i in range(20)]
    lvinv = [[ei[i][j] * expv[i] for j in range(20)] for i in range(20)]
    transt = [[0.0] * 20 for _ in range(20)]
    for i in range(20):
        for j in range(20):
            acc = 0.0
            for k in range(20):
                acc += cf[i][k] * lvinv[k][j]
            transt[i][j] = acc
    near_p, near_freq = np.zeros((20, 20), dtype), np.zeros((20, 20), dtype)
    for i in range(20):
        p, tot = [0.0] * 20, 0.0
        for j in range(20):
            p[j] = stat[j] * transt[i][j] * transt[i][j]
            tot += p[j]
        inv = 1.0 / tot
        for j in range(20):
            p[j] *= inv
        near_p[i] = p
        for j in range(20):
            p[j] /= stat[j]
        for j in range(20):
            rot = 0.0
            for k in range(20):
                rot += p[k] * cf[i][j]
            near_freq[i, j] = rot
    return near_p, near_freq


# ---- the operator case shared by tests/test_approxml_cpu.py (anchor, both outcomes) and tests/test_gpu_approxml.py (the device)
N_SEQS, N_POS, MAX_NODES = 5, 70, 16      # 70 columns: one past a 64-column pass of the quad workgroup
RATES = [0.5, 2.0]
CUSTOM, FIRST, SECOND = 5, (6, 7), (8, 9, 10)   # node ids: an uploaded vector profile, the first call's outputs, the second call's


def operator_case(model_tables, dtype, seed=3):
    """Leaves, one uploaded vector profile and two rounds of posteriors under `model_tables` (backend.aa_model_tables):
    dict(codes[5, 70], ratecat, custom=(w, c, f), calls=[[(out, a, b, len1, len2), ...], [...]]).
    Columns cycle through: the same code on both sides, different codes, code against gap, gap against gap; the second round joins
    vectors with vectors, a vector with a leaf, and the uploaded profile - mixtures a * e_x + (1 - a) * e_y with x a state of lane 3
    of a quad (3, 19) and y a state of another lane - with a leaf that is a gap or x."""
    rng = np.random.default_rng(seed)
    cf = np.asarray(model_tables["codefreq"], np.float64).reshape(21, 20)
    codes = np.full((N_SEQS, N_POS), NOCODE, np.uint8)
    x = rng.integers(0, 20, N_POS)
    y = (x + 1 + rng.integers(0, 19, N_POS)) % 20
    for p in range(N_POS):
        k = p % 4
        codes[0, p] = x[p] if k < 3 else NOCODE
        codes[1, p] = x[p] if k == 0 else y[p] if k == 1 else NOCODE
        codes[2, p] = x[p] if k != 1 else NOCODE                    # mostly agrees with leaf 0: dominant states one level up
        codes[3, p] = x[p] if p % 3 else y[p]
    w, c, f = np.ones(N_POS, dtype), np.full(N_POS, NOCODE, np.uint8), np.zeros((N_POS, 20), dtype)
    for p in range(N_POS):
        xs, ys, a = (3, 19)[p % 2], (5, 8, 14, 1)[p % 4], (0.97, 0.99, 0.9, 1.0)[(p // 2) % 4]
        f[p] = (a * cf[xs] + (1.0 - a) * cf[ys]).astype(dtype)
        codes[4, p] = NOCODE if p % 3 == 0 else xs
    calls = [[(6, 0, 1, 0.01, 0.1), (7, 2, 3, 0.1, 1.0)],
             [(8, 6, 7, 1.0, 0.01), (9, CUSTOM, 4, 0.01, 0.1), (10, 7, 0, 0.1, 0.1)]]
    return dict(codes=codes, ratecat=np.arange(N_POS) % 2, custom=(w, c, f), calls=calls)


def run_case(case, model_tables, dtype, near, limits):
    """every profile of the case through posterior(): {node: (w, c, f)}, {node: (what, ch, fail)}"""
    profs = {i: ((case["codes"][i] != NOCODE).astype(dtype), case["codes"][i].copy(), np.zeros((N_POS, 20), dtype)) for i in range(N_SEQS)}
    profs[CUSTOM] = case["custom"]
    notes = {}
    for call in case["calls"]:
        for out, a, b, l1, l2 in call:
            profs[out], *notes[out] = posterior(profs[a], profs[b], l1, l2, np.array(RATES, dtype), case["ratecat"], model_tables, near,
                                                limits[0], limits[1])
    return profs, notes
