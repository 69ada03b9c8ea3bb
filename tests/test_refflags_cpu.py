"""The one translation from the reference's flags to nj_newick's keywords (veryfasttree_amd/refflags.py) and the one constructor of
vft_nj_options (backend._nj_options).  No device."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import golden_util as G
from veryfasttree_amd import backend
from veryfasttree_amd.refflags import from_reference_flags, zero_round_stages

F32, F64 = np.float32, np.float64
FULL = dict(me_nni=True, spr=2, ml_nni=20)

# flags -> (n_codes, n_bootstrap, kwargs, other): everything the translation returns, written out
TABLE = [
    # the four rows of stages
    ("-nt -noml -nome", (4, 1000, dict(dtype=F32), {})),
    ("-nt -noml", (4, 1000, dict(dtype=F32, me_nni=True, spr=2), {})),
    ("-nt -nome -mllen", (4, 1000, dict(dtype=F32, mllen=20), {})),
    ("-nt", (4, 1000, dict(dtype=F32, **FULL), {})),
    ("-nt -nome", (4, 1000, dict(dtype=F32, ml_nni=20), {})),
    ("-nt -gtr -gamma", (4, 1000, dict(dtype=F32, gtr=True, gamma=True, **FULL), {})),
    ("-nt -nome -mllen -gtr", (4, 1000, dict(dtype=F32, mllen=20, gtr=True), {})),
    ("-nt -noml -spr 4", (4, 1000, dict(dtype=F32, me_nni=True, spr=4), {})),
    ("-nt -spr 0", (4, 1000, dict(dtype=F32, me_nni=True, spr=0, ml_nni=20), {})),
    # the thorough search
    ("-nt -spr 4 -mlacc 2 -slownni", (4, 1000, dict(dtype=F32, me_nni=True, spr=4, ml_nni=20, ml_accuracy=2, slow_nni=True), {})),
    ("-nt -nni 3 -mlnni 2 -sprlength 30", (4, 1000, dict(dtype=F32, nni_rounds=3, ml_nni_rounds=2, spr_length=30, **FULL), {})),
    ("-nt -nni 0", (4, 1000, dict(dtype=F32, ml_nni=20), {})),                     # no SPR round either (VeryFastTree.cpp:72)
    ("-nt -mlnni 0", (4, 1000, dict(dtype=F32, me_nni=True, spr=2), {})),          # -noml
    ("-nt -nome -mllen -mlacc 2", (4, 1000, dict(dtype=F32, mllen=20, ml_accuracy=2), {})),
    # -pseudo with and without a number
    ("-nt -noml -pseudo", (4, 1000, dict(dtype=F32, me_nni=True, spr=2, pseudo=1.0), {})),
    ("-nt -pseudo 0.5 -noml", (4, 1000, dict(dtype=F32, me_nni=True, spr=2, pseudo=0.5), {})),
    ("-nt -pseudo -noml -nome -nosupport", (4, 0, dict(dtype=F32, pseudo=1.0), {})),
    # the supports
    ("-nt -noml -nome -boot 100", (4, 100, dict(dtype=F32), {})),
    ("-nt -noml -nome -boot 100 -nosupport", (4, 0, dict(dtype=F32), {})),
    # proteins, precision, rate categories
    ("", (20, 1000, dict(dtype=F32, aa_model="jtt", **FULL), {})),
    ("-lg -double-precision", (20, 1000, dict(dtype=F64, aa_model="lg", **FULL), {})),
    ("-wag -nocat -nome -mllen", (20, 1000, dict(dtype=F32, aa_model="wag", mllen=1), {})),
    ("-nt -nome -nocat", (4, 1000, dict(dtype=F32, ml_nni=1), {})),
    ("-nt -double-precision -cat 5 -nome -mllen", (4, 1000, dict(dtype=F64, mllen=5), {})),
    ("-nt -cat 5", (4, 1000, dict(dtype=F32, me_nni=True, spr=2, ml_nni=5), {})),
    # the NJ phase, the schedule, and what nj_newick has no keyword for
    ("-nt -slow -noml -nome", (4, 1000, dict(dtype=F32, slow=True), {})),
    ("-nt -fastest -no2nd -noml -nome", (4, 1000, dict(dtype=F32, fastest=True, second_level=False), {})),
    ("-nt -fastest -threads 4 -seed 1", (4, 1000, dict(dtype=F32, fastest=True, second_level=False, threads=4, **FULL), dict(seed=1))),
    ("-nt -rawdist -makematrix", (4, 1000, dict(dtype=F32, **FULL), dict(rawdist=True, makematrix=True))),
    ("-nt -notop -noml -nome", (4, 1000, dict(dtype=F32), dict(notop=True))),
]


@pytest.mark.parametrize("flags,want", TABLE, ids=[t[0] or "(none)" for t in TABLE])
def test_the_table(flags, want):
    run = from_reference_flags(flags)
    assert (run.n_codes, run.n_bootstrap, run.kwargs, run.other) == want
    assert run.dtype == want[2]["dtype"]
    assert from_reference_flags(flags.split()) == run       # a list or a space-joined string


def test_threads_and_start_tree_beside_the_flags():
    run = from_reference_flags("-nt -noml", threads=4, intree_text="(a,b,(c,d));")
    assert run.kwargs == dict(dtype=F32, me_nni=True, spr=2, threads=4, intree="(a,b,(c,d));")
    assert from_reference_flags("-nt -noml -threads 4", threads=4).kwargs["threads"] == 4
    assert from_reference_flags("-nt -noml -intree t.nwk", intree_text="(a,b,(c,d));").kwargs["intree"] == "(a,b,(c,d));"
    with pytest.raises(ValueError, match="-threads"):
        from_reference_flags("-nt -threads 4", threads=2)
    with pytest.raises(ValueError, match="-intree"):
        from_reference_flags("-nt -intree t.nwk")            # (no file is opened here)


@pytest.mark.parametrize("flags,named", [
    ("-nt -bionj", "-bionj"), ("-nt in.fasta", "in.fasta"),                                             # unknown
    ("-nt -mlacc", "-mlacc"), ("-nt -mlacc -slownni", "-mlacc"), ("-nt -spr two", "-spr"), ("-boot", "-boot"), ("-nt -cat", "-cat"),
    ("-nt -mlnni 1.5", "-mlnni"), ("-nt -intree", "-intree"),                                          # the number is missing
    ("-nt -sprlength 65", "-sprlength"), ("-nt -sprlength 0", "-sprlength"), ("-nt -mlacc 0", "-mlacc"), ("-nt -nni -1", "-nni"),
    ("-nt -boot -3", "-boot"), ("-nt -cat 0", "-cat"), ("-nt -threads 0", "-threads"), ("-nt -spr -1", "-spr"),   # out of range
    ("-nt -pseudo -1", "-pseudo"), ("-nt -pseudo -0.5", "-pseudo"), ("-nt -pseudo nan", "-pseudo"), ("-nt -pseudo inf", "-pseudo"),
    ("-nt -nt", "-nt"), ("-nt -slow -fastest", "-slow"), ("-nt -lg", "-lg"), ("-lg -wag", "-wag"), ("-nt -nocat -cat 5", "-nocat"),
    ("-nt -2nd -no2nd", "-2nd")])
def test_what_cannot_be_translated_is_a_value_error_that_names_the_flag(flags, named):
    with pytest.raises(ValueError, match=re.escape(named)):
        from_reference_flags(flags)
    assert "64" in str(pytest.raises(ValueError, from_reference_flags, "-nt -sprlength 65").value)


def recorded_flags():
    """every `flags` / `r<k>_flags` entry of every fixture"""
    out = []
    for path in sorted(glob.glob(os.path.join(G.GOLDEN, "*.npz"))):
        with np.load(path) as d:
            out += [(os.path.basename(path)[:-4], key, bytes(d[key]).decode()) for key in d.files if re.fullmatch(r"(r\d+_)?flags", key)]
    return out


def test_every_recorded_command_line_translates():
    recorded = recorded_flags()
    assert len(recorded) > 150
    for name, key, flags in recorded:
        run = from_reference_flags(flags)
        assert run.n_codes == (4 if "-nt" in flags.split() else 20), (name, key)
        assert run.kwargs["dtype"] == (F64 if "-double-precision" in flags else F32), (name, key)
        assert ("makematrix" in run.other) == name.startswith("mm_"), (name, key)


def test_zero_rounds_are_the_switches():
    assert zero_round_stages(True, 2, 20, None, None) == (True, 2, 20)
    assert zero_round_stages(True, 2, 20, 3, 2) == (True, 2, 20)
    assert zero_round_stages(True, 2, 20, 0, None) == (False, 0, 20)
    assert zero_round_stages(True, 2, 20, None, 0) == (True, 2, 0)


# ------------------------------------------------------------------------------------------------ the options struct
# vft_nj_options as nj_newick with every keyword at its default hands it to C (include/vft_host.h has the reference's Options behind each)
DEFAULT_OPTIONS = dict(fastest=0, use_tophits_2nd=0, tophits_mult=1.0, tophits_close=-1.0, tophits_refresh=0.8, topvisible_mult=1.5, stale_out_limit=0.01,
                       f_reset_out_profile=0.02, n_reset_out_profile=200, tophits2_safety=3, tophits2_mult=1.0, tophits2_refresh=0.6, scoredist=0, mllen=0,
                       me_nni=0, ml_nni=0, spr=0, gtr=0, aa_model=0, comm=None, threads=1, debug_flags=0, gamma=0, out_profile_parts=0, slow=0, intree=None,
                       pseudo_weight=0.0, ml_accuracy=1, slow_nni=0, nni_rounds=0, ml_nni_rounds=0, spr_length=0)


def members(opt):
    return {name: getattr(opt, name) for name, _ in backend._NJOptions._fields_}


def test_the_constructor_has_the_defaults_member_for_member():
    assert members(backend._nj_options()) == DEFAULT_OPTIONS
    assert members(backend._nj_options(fastest=True)) == dict(DEFAULT_OPTIONS, fastest=1, use_tophits_2nd=1, tophits_refresh=0.5)
    assert members(backend._nj_options(fastest=True, use_tophits_2nd=False, tophits_refresh=0.7)) == dict(DEFAULT_OPTIONS, fastest=1, tophits_refresh=0.7)
    assert members(backend._nj_options(ml_accuracy=None, nni_rounds=None, threads=None)) == DEFAULT_OPTIONS       # None = the default
    got = members(backend._nj_options(aa_model="lg", intree="(a,b,(c,d));", pseudo_weight=0.5, me_nni=True, spr=4, spr_length=30))
    assert got == dict(DEFAULT_OPTIONS, aa_model=3, intree=b"(a,b,(c,d));", pseudo_weight=0.5, me_nni=1, spr=4, spr_length=30)
    with pytest.raises(TypeError, match="sprlength"):
        backend._nj_options(sprlength=30)                     # a misspelt member is no member


class Recorder:
    """stands where libvft_host.so would: keeps the vft_nj_options of the call and fails it, before anything looks at a context"""
    def __init__(self):
        self.options = []

    def record(self, *args):
        self.options += [members(a._obj) for a in args if isinstance(getattr(a, "_obj", None), backend._NJOptions)]
        return 1

    vft_nj_ml_newick = vft_nj_run = record


class NoDevice:
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    dt = np.dtype(np.float32)


def handed_to_c(monkeypatch, call):
    lib = Recorder()
    monkeypatch.setattr(backend, "load_host_library", lambda: lib)
    with pytest.raises(backend.VftError):
        call()
    assert len(lib.options) == 1
    return lib.options[0]


CODES = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
NAMES = ["s%d" % k for k in range(6)]


def test_nj_newick_hands_over_the_defaults_and_every_keyword_in_its_member(monkeypatch):
    newick = lambda **kw: handed_to_c(monkeypatch, lambda: backend.nj_newick(lambda n, L: NoDevice(), CODES, NAMES, **kw))
    assert newick() == DEFAULT_OPTIONS
    assert newick(fastest=True) == dict(DEFAULT_OPTIONS, fastest=1, use_tophits_2nd=1, tophits_refresh=0.5)
    # the slip a positional fill invites: a value one slot off
    run = from_reference_flags("-nt -spr 4 -mlacc 2 -slownni")
    got = newick(me_lengths=True, **run.kwargs)
    assert (got["spr"], got["ml_accuracy"], got["slow_nni"]) == (4, 2, 1)
    assert got == dict(DEFAULT_OPTIONS, me_nni=1, ml_nni=20, spr=4, ml_accuracy=2, slow_nni=1)
    got = newick(fastest=True, second_level=False, scoredist=True, mllen=3, me_nni=True, ml_nni=7, spr=4, gtr=True, aa_model="lg", threads=5,
                 debug_flags=128, gamma=True, out_profile_parts=3, slow=True, intree="(a,b);", pseudo=0.5, ml_accuracy=2, slow_nni=True, nni_rounds=3,
                 ml_nni_rounds=2, spr_length=30)
    assert got == dict(DEFAULT_OPTIONS, fastest=1, tophits_refresh=0.5, scoredist=1, mllen=3, me_nni=1, ml_nni=7, spr=4, gtr=1, aa_model=3, threads=5,
                       debug_flags=128, gamma=1, out_profile_parts=3, slow=1, intree=b"(a,b);", pseudo_weight=0.5, ml_accuracy=2, slow_nni=1,
                       nni_rounds=3, ml_nni_rounds=2, spr_length=30)
    # nni_rounds=0 / ml_nni_rounds=0 keep their meaning
    assert newick(nni_rounds=0, ml_nni_rounds=0, **FULL) == DEFAULT_OPTIONS


def test_nj_run_hands_over_its_keywords_in_their_members(monkeypatch):
    run = lambda **kw: handed_to_c(monkeypatch, lambda: backend.nj_run(NoDevice(), CODES, **kw))
    assert run() == dict(DEFAULT_OPTIONS, ml_accuracy=0)            # (the members behind intree stay zero here, as they always were)
    got = run(fastest=True, tophits_refresh=0.7, second_level=False, scoredist=True, aa_model="wag", tophits_mult=-1.0, debug_flags=3,
              out_profile_parts=2, slow=True, intree="(a,b);")
    assert got == dict(DEFAULT_OPTIONS, ml_accuracy=0, fastest=1, tophits_refresh=0.7, scoredist=1, aa_model=2, tophits_mult=-1.0, debug_flags=3,
                       out_profile_parts=2, slow=1, intree=b"(a,b);")
