"""`-slow` (exhaustive neighbour joining) on the CPU oracle: the rule of tests/nj_slow_py.py - a kept distance per pair, the
criterion formed anew at every join, ties to the first (i, j) - against the reference's own `Join` lines
(tests/golden/slow_*.npz, produced by tools/gen_slow_fixtures.py from `VeryFastTree -slow -threads 1 -verbose 3`).  Guards the
fixtures and the rule without a GPU; tests/test_gpu_nj_slow.py runs the product against the same fixtures."""
import numpy as np
import pytest

import golden_util as G
from oracle_ops import OracleOps
from nj_slow_py import SlowNJDriver
from test_nj_driver_cpu import unique_codes


def run_oracle(name):
    d = G.load(name)
    codes = unique_codes(d["codes"])
    ops = OracleOps(codes.shape[0], codes.shape[1], 4, np.float64 if "double" in name else np.float32)
    drv = SlowNJDriver(ops, codes)
    joins = drv.run()
    return d, drv, np.array([(a, b, c) for a, b, c, _ in joins], dtype=np.int64), np.array([c for _, _, _, c in joins])


@pytest.mark.parametrize("name", ["slow_nt_200", "slow_nt_mirror", "slow_nt_mirror_double", "slow_nt_5", "slow_nt_4"])
def test_exhaustive_join_order_matches_reference(name):
    d, drv, got, crit = run_oracle(name)
    want = d["joins"]
    assert len(got) == len(want) == len(unique_codes(d["codes"])) - 3
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "first differing join %d: got %s want %s" % (bad[0], got[bad[0]], want[bad[0]])
    assert np.allclose(crit, d["join_criterion"], atol=1e-6)   # printed with %.6f
    if "mirror" in name:
        # the mirrored alignment is there for exact ties: the fixture must go on testing the first-(i, j) rule
        assert len(drv.tied_joins) >= 1, "no join of %s has a tied minimum" % name


def test_slow_fixtures_differ_from_the_default_search():
    """-slow must not be a case the heuristics already cover: the order parts from bb_nt_200's"""
    slow, fast = G.load("slow_nt_200"), G.load("bb_nt_200")
    assert np.array_equal(slow["codes"], fast["codes"])
    assert not np.array_equal(slow["joins"], fast["joins"])
