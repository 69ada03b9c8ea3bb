"""The thorough search (`-mlacc N`, `-slownni`, `-nni N`, `-mlnni N`, `-sprlength N`), the host half: the command line of
tools/nj_tree.py, the refusals of the driver, the arithmetic of the round counts and the SPR spacing (vft_nj_round_plan) against the
reference's formulas restated here (VeryFastTreeImpl.tcc:145-149, :187-204, :345), and the fixtures (tools/gen_thorough_fixtures.py).
No device."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {"thor_nt_150": 8, "thor_nt_60_gtr": 2, "thor_aa_60_lg": 3, "thor_aa_40_wag_double": 2, "thor_nt_400_noisy": 5,
            "thor_aa_150_noisy": 1, "thor_nt_30_x2200": 1, "thor_aa_24_x600_lg": 1, "thor_nt_300_chains": 2, "thor_nt_150_mllen": 2}   # name: runs
NEW_FLAGS = ("-mlacc", "-slownni", "-nni", "-mlnni", "-sprlength")


def load_tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import nj_tree
    return nj_tree


# ------------------------------------------------------------------------------------------------ the tool
def asked(t, args):
    """what tools/nj_tree.py hands to nj_newick for `args`, the thorough-search keywords and the stages they touch only"""
    kw = t.translate(args)[1].kwargs
    return {key: kw[key] for key in ("ml_accuracy", "slow_nni", "nni_rounds", "ml_nni_rounds", "spr_length", "me_nni", "spr", "ml_nni") if key in kw}


FULL = dict(me_nni=True, spr=2, ml_nni=20)   # the stages of -full


def test_the_tool_parses_the_options():
    t = load_tool()
    assert asked(t, ["in.fa", "-full"]) == FULL
    assert asked(t, ["in.fa", "-full", "-spr", "4", "-mlacc", "2", "-slownni"]) == \
        dict(FULL, spr=4, ml_accuracy=2, slow_nni=True)                                 # (-spr is not -sprlength)
    assert asked(t, ["in.fa", "-nni", "3", "-full", "-mlnni", "2", "-sprlength", "30"]) == \
        dict(FULL, nni_rounds=3, ml_nni_rounds=2, spr_length=30)
    assert asked(t, ["in.fa", "-full", "-nni", "0", "-mlnni", "0"]) == {}
    assert asked(t, ["in.fa", "-full", "-sprlength", "64"])["spr_length"] == 64
    for bad in (["-mlacc"], ["-mlacc", "0"], ["-mlacc", "-1"], ["-mlacc", "two"], ["-nni", "-1"], ["-mlnni", "1.5"], ["-sprlength", "0"],
                ["-sprlength", "65"], ["-nni", "-full"]):
        for mode in ([], ["-full"]):
            with pytest.raises(SystemExit) as e:
                t.translate(["in.fa"] + mode + bad)
            assert bad[0] in str(e.value), bad
    assert "64" in str(pytest.raises(SystemExit, t.translate, ["in.fa", "-full", "-sprlength", "65"]).value)


def test_the_tool_maps_zero_rounds_onto_the_existing_switches():
    t = load_tool()
    assert asked(t, ["in.fa", "-full", "-nni", "0"]) == dict(ml_nni=20)                         # `-nni 0` also sets spr = 0
    assert asked(t, ["in.fa", "-full", "-mlnni", "0"]) == dict(me_nni=True, spr=2)              # `-mlnni 0` is -noml
    assert asked(t, ["in.fa", "-full", "-nni", "3", "-mlnni", "2", "-mlacc", "2", "-slownni", "-sprlength", "5"]) == \
        dict(FULL, nni_rounds=3, ml_nni_rounds=2, ml_accuracy=2, slow_nni=True, spr_length=5)
    assert asked(t, ["in.fa"]) == {}
    # the rule itself, as nj_newick applies it to nni_rounds=0 / ml_nni_rounds=0
    from veryfasttree_amd.refflags import zero_round_stages
    assert zero_round_stages(True, 2, 20, 0, None) == (False, 0, 20) and zero_round_stages(True, 2, 20, None, 0) == (True, 2, 0)
    assert zero_round_stages(True, 2, 20, 3, 2) == zero_round_stages(True, 2, 20, None, None) == (True, 2, 20)


def test_the_tool_refuses_an_option_without_its_stage():
    t = load_tool()
    for key, flag in (("ml_accuracy", "-mlacc"), ("slow_nni", "-slownni"), ("nni_rounds", "-nni"), ("ml_nni_rounds", "-mlnni"),
                      ("spr_length", "-sprlength")):
        option = [flag] if flag == "-slownni" else [flag, "1"]
        with pytest.raises(SystemExit) as e:
            t.translate(["in.fa"] + option)
        assert flag in str(e.value) and "-full" in str(e.value)
        if key != "ml_accuracy":                       # -mllen runs no NNI and no SPR round
            with pytest.raises(SystemExit):
                t.translate(["in.fa", "-mllen"] + option)
    # the supports and the -gtr fit of -mllen read the accuracy (NJ.tcc:6934, :6462)
    assert asked(t, ["in.fa", "-mllen", "-mlacc", "2"]) == dict(ml_accuracy=2)


# ------------------------------------------------------------------------------------------------ the driver's refusals
class NoDevice:
    """stands where a context would: the refusals below come before anything looks at it"""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)


def newick_without_a_device(**kw):
    from veryfasttree_amd import backend
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    return backend.nj_newick(lambda n, L: NoDevice(), codes, ["s%d" % k for k in range(6)], me_lengths=True, me_nni=True, spr=2, **kw)


@pytest.mark.parametrize("key,flag", [("ml_accuracy", "-mlacc"), ("slow_nni", "-slownni"), ("nni_rounds", "-nni"), ("ml_nni_rounds", "-mlnni"),
                                      ("spr_length", "-sprlength")])
def test_the_driver_refuses_a_negative_member_before_the_device(key, flag):
    from veryfasttree_amd.backend import VftError
    for bad in (-1, -2 ** 31):
        with pytest.raises(VftError, match=r"vft_nj_options\.%s \(%s\) is negative" % (key, flag)):
            newick_without_a_device(**{key: bad})


def test_the_driver_refuses_chains_beyond_its_buffers_before_the_device():
    from veryfasttree_amd.backend import VftError
    for bad in (65, 1000):
        with pytest.raises(VftError, match=r"vft_nj_options\.spr_length \(-sprlength\) is above 64: the chain buffers of MLLengths::sprAttempt hold 64 steps"):
            newick_without_a_device(spr_length=bad)


def test_the_earlier_refusals_stay():
    from veryfasttree_amd.backend import VftError
    with pytest.raises(VftError, match="-slow with me_nni, spr or ml_nni is not built"):
        newick_without_a_device(slow=True, ml_accuracy=2, slow_nni=True)
    with pytest.raises(VftError, match="-pseudo takes a finite weight >= 0"):
        newick_without_a_device(pseudo=-1.0, spr_length=5)


def test_the_struct_ends_with_the_five_members():
    from veryfasttree_amd import backend
    names = [f[0] for f in backend._NJOptions._fields_]
    assert names[-6:] == ["pseudo_weight", "ml_accuracy", "slow_nni", "nni_rounds", "ml_nni_rounds", "spr_length"]
    text = open(os.path.join(ROOT, "include", "vft_host.h")).read()
    body = text[text.index("typedef struct {\n    int32_t fastest;"):text.index("} vft_nj_options;")]
    declared = re.findall(r"^    (?:const )?\w+ \*?(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
    assert declared == names


# ------------------------------------------------------------------------------------------------ the rounds
def restated_plan(n, nni, mlnni, spr):
    """VeryFastTreeImpl.tcc:145-149 and the loop of :161-204: the NNI rounds behind which each SPR round runs"""
    nni_to_do = int(0.5 + 4.0 * math.log(n) / math.log(2)) if nni is None else nni
    ml_to_do = mlnni if mlnni is not None else int(0.5 + 2.0 * math.log(n) / math.log(2))
    behind, remaining = [], spr
    for i in range(nni_to_do):
        if remaining > 0 and nni_to_do // (spr + 1) > 0 and (i + 1) % (nni_to_do // (spr + 1)) == 0:
            behind.append(i + 1)
            remaining -= 1
    behind += [nni_to_do] * remaining          # "do any remaining SPR rounds"
    return nni_to_do, ml_to_do, ml_to_do - 2, behind


@pytest.mark.parametrize("spr", [0, 2, 4])
@pytest.mark.parametrize("nni", [None, 1, 3, 5])
def test_round_counts_and_spr_spacing(nni, spr):
    from veryfasttree_amd.backend import round_plan
    for n in (4, 24, 150, 400, 1000000):
        for mlnni in (None, 1, 2, 7):
            assert round_plan(n, nni, mlnni, spr) == restated_plan(n, nni, mlnni, spr), (n, nni, mlnni, spr)
    # what the formula means for the cases at hand
    if nni == 1:
        assert round_plan(150, nni, None, spr)[3] == [1] * spr             # 1 / (spr + 1) == 0: every SPR round behind the only NNI round
    if nni == 3 and spr == 2:
        assert round_plan(150, nni, None, spr)[3] == [1, 2]
    if nni == 5 and spr == 4:
        assert round_plan(150, nni, None, spr)[3] == [1, 2, 3, 4]
    if nni == 5 and spr == 2:
        assert round_plan(150, nni, None, spr)[3] == [1, 2]
    if nni == 3 and spr == 4:
        assert round_plan(150, nni, None, spr)[3] == [3, 3, 3, 3]


def test_default_round_counts():
    from veryfasttree_amd.backend import round_plan
    assert round_plan(150, None, None, 2)[:3] == (29, 14, 12)
    assert round_plan(150, None, 2, 2)[1:3] == (2, 0)          # `-mlnni 2`: the statistics are reset behind the first round
    assert round_plan(150, None, 1, 2)[1:3] == (1, -1)         # never


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixtures_load_and_differ_from_their_controls(name):
    d = G.load(name)
    assert int(d["n_runs"]) == FIXTURES[name]
    strip = lambda t: re.sub(rb"\)[0-9.]+:", b"):", re.sub(rb":[0-9.eE+-]+", b":", t))
    for k in range(FIXTURES[name]):
        pre = "r%d_" % k
        flags = bytes(d[pre + "flags"]).decode().split()
        expect = bytes(d[pre + "expect"]).decode()
        assert any(f in flags for f in NEW_FLAGS) and int(d[pre + "threads"]) in (1, 4)
        got, ctl = bytes(d[pre + "newick"]), bytes(d[pre + "control_newick"])
        gots, ctls = bytes(d[pre + "newick_support"]), bytes(d[pre + "control_newick_support"])
        for t in (got, ctl, gots, ctls):
            assert t.strip().endswith(b";")
        if expect == "equal":
            assert flags[-2:] == ["-sprlength", "30"] and got == ctl and gots == ctls
        elif expect == "supports":                      # `-mllen -mlacc 2`: the second pass of the SH-like supports is all that changes
            assert "-mllen" in flags and got == ctl and gots != ctls, (name, k)
        else:
            assert expect in ("differs", "topology") and got != ctl and gots != ctls, (name, k)
        if expect == "topology":
            assert strip(got) != strip(ctl), (name, k)
        if "-noml" not in flags:
            assert len(d[pre + "loglk"]) >= 1 and len(d[pre + "rates"]) == 20 and len(d[pre + "ratecat"]) == d["codes"].shape[1]
            assert len(d[pre + "control_loglk"]) >= 1
