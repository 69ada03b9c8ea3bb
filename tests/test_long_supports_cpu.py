"""The lsup_* fixtures (tools/gen_longsupport_fixtures.py: local supports beyond 1 706 columns) and the -boot option of tools/nj_tree.py,
without a device."""
import importlib.util
import os
import re

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (sequences, columns, states)
LSUP = {"lsup_nt_16x1707": (16, 1707, 4), "lsup_nt_16x1707_boot100": (16, 1707, 4), "lsup_nt_12x3414_double": (12, 3414, 4),
        "lsup_nt_12x5121_me": (12, 5121, 4), "lsup_nt_8x10224": (8, 10224, 4), "lsup_aa_12x2000": (12, 2000, 20),
        "lsup_aa_10x3500_double": (10, 3500, 20), "lsup_nt_14x2400_gappy": (14, 2400, 4)}


def group_labels(tree):
    return re.findall(r"\)([0-9.]+):", tree)


@pytest.mark.parametrize("name", sorted(LSUP))
def test_fixture_loads_and_its_tree_parses(name):
    n, L, nc = LSUP[name]
    d = G.load(name)
    codes = d["codes"]
    assert codes.shape == (n, L) and codes.dtype == np.uint8
    assert int(codes[codes != G.NOCODE].max()) < nc
    assert len({r.tobytes() for r in codes}) == n   # no duplicates: every row is a leaf
    flags = bytes(d["flags"]).decode().split()
    assert "-noml" in flags and ("-nt" in flags) == (nc == 4)
    for key in ("nj_newick", "me_lengths", "newick_support"):
        text = bytes(d[key]).decode().strip()
        assert text.endswith(";") and text.count("(") == text.count(")") == n - 2   # a root of three over n leaves
        assert sorted(re.findall(r"[(,](s\d+):", text)) == sorted("s%d" % k for k in range(n))
    assert not group_labels(bytes(d["nj_newick"]).decode()) and not group_labels(bytes(d["me_lengths"]).decode())
    sup = group_labels(bytes(d["newick_support"]).decode())
    assert len(sup) == n - 3
    assert all(re.fullmatch(r"[01]\.\d{3}", s) and 0.0 <= float(s) <= 1.0 for s in sup)
    assert len(set(sup)) == int(d["n_distinct_supports"]) >= 3
    if "-boot" in flags:   # 100 resamples: supports are hundredths
        assert flags[flags.index("-boot") + 1] == "100" and all(s.endswith("0") for s in sup)


def test_the_two_1707_fixtures_share_their_alignment_and_lengths():
    a, b = G.load("lsup_nt_16x1707"), G.load("lsup_nt_16x1707_boot100")
    assert np.array_equal(a["codes"], b["codes"])
    assert bytes(a["me_lengths"]) == bytes(b["me_lengths"])
    assert bytes(a["newick_support"]) != bytes(b["newick_support"])


def test_gappy_fixture_has_pairs_without_a_common_column():
    codes = G.load("lsup_nt_14x2400_gappy")["codes"]
    have = codes != G.NOCODE
    assert not (have[0:3].any(0) & have[3:6].any(0)).any()
    assert have[0:3, :300].any() and have[3:6, 2100:].any() and have[6:].mean() > 0.9


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("nj_tree_tool", os.path.join(ROOT, "tools", "nj_tree.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_boot_option_parsing(tool):
    n_boot = lambda args: tool.translate(args)[1].n_bootstrap
    assert n_boot(["in.fa"]) == 1000
    assert n_boot(["in.fa", "-boot", "100"]) == 100
    assert n_boot(["in.fa", "-double", "-boot", "1"]) == 1
    assert n_boot(["in.fa", "-boot", "1001", "-mllen"]) == 1001
    # -boot 0 is -nosupport; -nosupport and -nj-lengths win over a count
    assert n_boot(["in.fa", "-boot", "0"]) == n_boot(["in.fa", "-nosupport"]) == 0
    assert n_boot(["in.fa", "-boot", "100", "-nosupport"]) == 0
    assert n_boot(["in.fa", "-boot", "100", "-nj-lengths"]) == 0


@pytest.mark.parametrize("args", [["in.fa", "-boot"], ["in.fa", "-boot", "ten"], ["in.fa", "-boot", "2.5"], ["in.fa", "-boot", "-3"],
                                  ["in.fa", "-boot", "-nosupport"]])
def test_boot_option_rejects_what_is_no_count(tool, args):
    with pytest.raises(SystemExit) as e:
        tool.translate(args)
    assert "-boot" in str(e.value)
