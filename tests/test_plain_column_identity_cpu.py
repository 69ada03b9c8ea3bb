"""The identity behind the plain-column path of vft_int_chunk_consume_prof (csrc/vft_kernels_nj.h), in numpy, in both precisions.

A query column that holds a plain code c has the exact one-hot of c as its frequency vector.  Against a target column (weight w_t,
vector f_t: finite, not negative) the kernel's full expression

    ww = wq * w_t;  wgt = (double) ww;  pr[k] = onehot[k] * f_t[k];  piece = (((1 - pr[0]) - pr[1]) - pr[2]) - pr[3]   (in double)

and the short one, piece = 1 - (double) f_t[c], give the same bits for wgt and for wgt * piece.  And a padding column (weight 0 on both
sides) adds +0.0 to both running sums, which changes no sum - a sum that is +0 included - so a group of padding columns may be skipped.
"""
import numpy as np
import pytest

DTYPES = [np.float32, np.float64]


def _values(dt, rng, n):
    """finite, non-negative: the special ones and random ones of every magnitude"""
    fi = np.finfo(dt)
    special = [0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, fi.tiny, fi.tiny / 2, float(fi.smallest_subnormal), 5 * float(fi.smallest_subnormal),
               1.0 - fi.epsneg, 1.0 - 2 * fi.epsneg, 1.0 + fi.eps, 0.75, 2.0 / 3.0, 1e-3, 0.999]
    rnd = np.concatenate([rng.random(n), rng.random(n) * 1e-6, 1.0 - rng.random(n) * 1e-6, np.exp(rng.uniform(np.log(float(fi.tiny)) - 5, 0.0, n))])
    v = np.concatenate([np.asarray(special, np.float64), rnd]).astype(dt)
    v = np.abs(v)   # (+0, never -0)
    assert np.all(np.isfinite(v)) and not np.any(np.signbit(v))
    return v


def _bits(x):
    assert x.dtype == np.float64
    return np.ascontiguousarray(x).view(np.uint64)


def _full(wq, wt, ft, onehot):
    ww = wq * wt                       # the precision's product
    assert ww.dtype == wq.dtype
    wgt = ww.astype(np.float64)
    pr = onehot * ft                   # the precision's products
    assert pr.dtype == wq.dtype
    piece = np.float64(1.0) - pr[..., 0].astype(np.float64)
    piece = piece - pr[..., 1].astype(np.float64)
    piece = piece - pr[..., 2].astype(np.float64)
    piece = piece - pr[..., 3].astype(np.float64)
    return wgt, wgt * piece


def _short(wq, wt, ft, code):
    ww = wq * wt
    wgt = ww.astype(np.float64)
    piece = np.float64(1.0) - ft[..., code].astype(np.float64)
    return wgt, wgt * piece


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("code", range(4))
def test_plain_query_column_full_and_short_expression_same_bits(dt, code):
    rng = np.random.default_rng(100 + code)
    v = _values(dt, rng, 200)
    m = 60000
    wq = v[rng.integers(0, len(v), m)]
    wt = v[rng.integers(0, len(v), m)]
    ft = v[rng.integers(0, len(v), (m, 4))]
    # every special value against every special value too, in the selected entry and in the others
    sp = v[:16]
    g = np.stack(np.meshgrid(sp, sp, sp, indexing="ij"), -1).reshape(-1, 3)
    ft_g = np.stack([g[:, 1]] * 4, 1)
    ft_g[:, code] = g[:, 2]
    wq, wt, ft = np.concatenate([wq, g[:, 0]]), np.concatenate([wt, sp[rng.integers(0, 16, len(g))]]), np.concatenate([ft, ft_g])
    onehot = np.zeros(4, dt)
    onehot[code] = 1
    with np.errstate(under="ignore"):
        wgt_f, term_f = _full(wq, wt, ft, onehot)
        wgt_s, term_s = _short(wq, wt, ft, code)
    assert np.array_equal(_bits(wgt_f), _bits(wgt_s))
    assert np.array_equal(_bits(term_f), _bits(term_s))
    # the three idle products are +0, not -0, whatever f_t holds
    pr = onehot * ft
    idle = np.delete(pr, code, axis=1)
    assert np.all(idle == 0) and not np.any(np.signbit(idle))


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_padding_column_adds_nothing(dt):
    """a padding column: wq = w_t = 0, both vectors 0 (the query's is what vft_extract_query stages beyond nPos)"""
    zero = np.zeros(1, dt)
    wgt, term = _full(zero, zero, np.zeros((1, 4), dt), np.zeros(4, dt))
    assert _bits(wgt)[0] == 0 and _bits(term)[0] == 0            # +0.0 and +0.0 * 1.0 = +0.0
    rng = np.random.default_rng(7)
    fi = np.finfo(np.float64)
    sums = np.concatenate([[0.0, fi.tiny, float(fi.smallest_subnormal), 1.0, 200.0, 1e300], rng.random(1000) * 200.0,
                           _values(dt, rng, 50).astype(np.float64)])
    assert not np.any(np.signbit(sums))
    for s in (sums + wgt[0], sums + term[0]):
        assert np.array_equal(_bits(s), _bits(sums))
    # eight of them in a row (a skipped group)
    acc = sums.copy()
    for _ in range(8):
        acc = acc + term[0]
    assert np.array_equal(_bits(acc), _bits(sums))
