"""The two identities behind the seed code records of the multi-seed sweeps (vft_int_chunk_consume_all, vft_usel_code in
csrc/vft_kernels_nj.h), in numpy, in both precisions.

MASKS.  A column's record is a dword with one code byte per seed: byte q holds seed q's code, 0..3, or 127 (NOCODE) at a gap and in
bytes no seed owns.  The kernel selects f_t[c] with two lane masks, all-ones or zero: the arithmetic sign-extensions of bits 8q and
8q + 1 of the dword (s_bfe_i64, width 1).  They must be (c & 1) and (c & 2) as all-ones / zero whatever the other three bytes hold, and
bit 8q + 6 must be set for 127 and for no code.

GAPS.  At a gap of a leaf seed the pair's weight is +0.0 (w_t * 0.0, w_t finite and not negative): it adds +0.0 to denom and
(+0.0) * piece to top, piece = 1 - (double) f_t[c].  Neither changes the bit pattern of a running sum (which is never -0.0), so the pair
may be skipped.
"""
import itertools

import numpy as np
import pytest

DTYPES = [np.float32, np.float64]
CODES = [0, 1, 2, 3, 127]
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _sext_bit(w, b):
    """s_bfe_i64 with width 1: bit b of the 64-bit operand, sign-extended - as shifts on int64 (numpy's >> on a signed type is arithmetic)"""
    w = np.asarray(w, np.uint64)
    return ((w << np.uint64(63 - b)).view(np.int64) >> np.int64(63)).view(np.uint64)


def _records():
    """every dword of four bytes from CODES: every code in every byte lane beside every combination of the others"""
    return np.array([sum(c << (8 * q) for q, c in enumerate(cs)) for cs in itertools.product(CODES, repeat=4)], np.uint64)


@pytest.mark.parametrize("half", [0, 1], ids=["even_column", "odd_column"])
@pytest.mark.parametrize("q", range(4))
def test_masks_are_sign_extended_bits_of_the_code_byte(q, half):
    """an even column's dword is the low half of its 64-bit word, an odd column's the high half; the other half holds any record"""
    recs = _records()
    other = recs[::-1]
    w = recs << np.uint64(32) | other if half else other << np.uint64(32) | recs
    off = 32 * half + 8 * q
    c = (recs >> np.uint64(8 * q)) & np.uint64(0xFF)
    assert set(c.tolist()) == set(CODES)
    m0, m1 = _sext_bit(w, off), _sext_bit(w, off + 1)
    assert np.array_equal(m0, np.where(c & np.uint64(1), ALL_ONES, np.uint64(0)))
    assert np.array_equal(m1, np.where(c & np.uint64(2), ALL_ONES, np.uint64(0)))
    gap = (w >> np.uint64(off + 6)) & np.uint64(1)
    assert np.array_equal(gap == 1, c == 127)
    # the select the masks drive, m1 ? (m0 ? f[3] : f[2]) : (m0 ? f[1] : f[0]), is f[c] for a code (and f[3] at a gap: never used)
    f = np.array([10, 11, 12, 13])
    lo, hi = np.where(m0 != 0, f[1], f[0]), np.where(m0 != 0, f[3], f[2])
    sel = np.where(m1 != 0, hi, lo)
    assert np.array_equal(sel, f[np.minimum(c, np.uint64(3)).astype(np.int64)])


def test_the_zero_extended_profile_record():
    """profile seeds: the dword is zero-extended to 64 bits; the same bits, the high half never read"""
    recs = _records()
    for q in range(4):
        c = (recs >> np.uint64(8 * q)) & np.uint64(0xFF)
        assert np.array_equal(_sext_bit(recs, 8 * q) != 0, (c & np.uint64(1)) != 0)
        assert np.array_equal(_sext_bit(recs, 8 * q + 1) != 0, (c & np.uint64(2)) != 0)


def _bits(x):
    assert x.dtype == np.float64
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_gap_pair_adds_nothing(dt):
    fi, fd = np.finfo(dt), np.finfo(np.float64)
    rng = np.random.default_rng(5)
    # f_t[c]: 0, 1, 1/2, denormals, values next to 1 on both sides (piece slightly negative), random ones
    ft = np.concatenate([np.array([0.0, 1.0, 0.5, fi.tiny, fi.tiny / 2, float(fi.smallest_subnormal), 1.0 - fi.epsneg, 1.0 + fi.eps,
                                   1.0 + 4 * fi.eps, 0.25, 1.0 / 3.0]), rng.random(500)]).astype(dt)
    piece = np.float64(1.0) - ft.astype(np.float64)
    assert np.any(piece < 0) and np.any(piece == 0) and np.any(piece == 1) and np.all(np.isfinite(piece))
    # the target's weight times the gap factor 0.0: +0.0 for every finite weight that is not negative
    wt = np.concatenate([np.array([0.0, 1.0, 0.5, fi.tiny, float(fi.smallest_subnormal), 1.0 - fi.epsneg]), rng.random(100)]).astype(dt)
    wgt = wt.astype(np.float64) * np.float64(0.0)
    assert np.all(_bits(wgt) == 0)
    term = np.float64(0.0) * piece                    # +0.0 or, for a negative piece, -0.0
    assert np.all(term == 0) and np.any(np.signbit(term)) and not np.all(np.signbit(term))
    # running sums: +0.0, denormal, ordinary, large - never -0.0
    sums = np.concatenate([[0.0, float(fd.smallest_subnormal), 5 * float(fd.smallest_subnormal), fd.tiny, float(fi.smallest_subnormal),
                            0.01, 1.0, 37.0, 200.0, 1e6, 1e300, fd.max], rng.random(500) * 200.0])
    assert not np.any(np.signbit(sums))
    denom = sums + np.float64(0.0)
    assert np.array_equal(_bits(denom), _bits(sums))
    top = sums[:, None] + term[None, :]
    assert np.array_equal(_bits(top), np.broadcast_to(_bits(sums)[:, None], top.shape))
    # a whole group of gapped columns
    acc = sums.copy()
    for t in term[:8]:
        acc = acc + t
    assert np.array_equal(_bits(acc), _bits(sums))
