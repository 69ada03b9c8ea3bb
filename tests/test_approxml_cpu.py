"""`-approxml` without a device: the near-constant posterior tables of the host driver, the numpy restatement of one posterior that the
GPU tests compare the kernels with (anchored on the CPU oracle first), the translation of the flag, the one call nj_newick adds, and
the fixtures."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import approx_posterior_np as R
import golden_util as G
from oracle import Oracle, tolerances
from veryfasttree_amd import backend
from veryfasttree_amd.refflags import from_reference_flags

F32, F64 = np.float32, np.float64
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G.GOLDEN, "approx_aa_*.npz")))


@pytest.fixture(scope="module", autouse=True)
def built():
    from veryfasttree_amd import build
    build.build()


@pytest.mark.parametrize("model", ["jtt", "wag", "lg"])
@pytest.mark.parametrize("dt,tag", [(F32, "f32"), (F64, "f64")])
def test_near_tables_equal_the_restatement(model, dt, tag):
    """host/AAModels.h nearPosteriorTables against TransitionMatrix.tcc:227-279 restated in Python floats from the tables the REFERENCE
    built (wb_aa_tables.npz): same libm, same order of operations - equal, not close"""
    d = G.load("wb_aa_tables")
    key = lambda k: d["%s.%s.%s" % (model, tag, k)]
    want_p, want_f = R.near_tables(key("stat"), key("eigenval"), key("codefreq"), key("eigeninv"))
    got = backend.aa_near_tables(model, dt)
    assert want_p.dtype == dt
    assert np.array_equal(got["nearP"].astype(dt), want_p)
    assert np.array_equal(got["nearFreq"].astype(dt), want_f)
    assert np.array_equal(got["nearP"].astype(dt).astype(np.float64), got["nearP"])   # numeric_t values held in double
    # what the tables are: a distribution per row whose own state dominates
    assert np.allclose(want_p.sum(1), 1.0, atol=1e-6) and (want_p.argmax(1) == np.arange(20)).all()


def model_of(dt):
    t = backend.aa_model_tables("lg", dt)
    n = backend.aa_near_tables("lg", dt)
    return t, (n["nearP"], n["nearFreq"])


@pytest.fixture(scope="module", params=[F32, F64], ids=["f32", "f64"])
def case(request):
    dt = np.dtype(request.param)
    t, near = model_of(dt)
    c = R.operator_case(t, dt)
    limits = tolerances(dt)
    exact, _ = R.run_case(c, t, dt, None, limits)
    rough, notes = R.run_case(c, t, dt, near, limits)
    return dict(dt=dt, t=t, near=near, c=c, limits=limits, exact=exact, rough=rough, notes=notes)


def test_the_restatement_without_the_flag_is_the_oracle_bit_for_bit(case):
    """the anchor: a restatement that misses this is wrong, whatever the device says"""
    dt, t, c = case["dt"], case["t"], case["c"]
    orc = Oracle(dt)
    tm = orc.tmat(t["stat"], t["statinv"], t["eigenval"], t["codefreq"], t["eigeninv"], t["eigeninvT"])
    profs = {i: orc.leaf_profile(c["codes"][i], 20) for i in range(R.N_SEQS)}
    profs[R.CUSTOM] = tuple(np.ascontiguousarray(x) for x in c["custom"])
    n = 0
    for call in c["calls"]:
        for out, a, b, l1, l2 in call:
            profs[out] = orc.posterior_profile(profs[a], profs[b], l1, l2, np.array(R.RATES, dt), c["ratecat"], tm, case["limits"][0], case["limits"][1])
            got = case["exact"][out]
            assert np.array_equal(got[0], profs[out][0]) and np.array_equal(got[1], profs[out][1]), out
            assert np.array_equal(got[2].view(np.uint8), profs[out][2].view(np.uint8)), out
            n += 1
    assert n == 5


def test_the_case_takes_every_branch(case):
    """both outcomes in every posterior the device will be asked for, and the quad kernels' hard column: the dominant state owned by
    lane 3 of a quad (j = 3 or 19), the ratio test failing at a state of another lane"""
    what = np.concatenate([case["notes"][k][0] for k in R.FIRST + R.SECOND])
    assert (what == R.ROUGH).sum() >= 10 and (what == R.GAVE_UP).sum() >= 3 and (what == R.NEVER).sum() >= 10 and (what == R.GAP).sum() >= 1
    for k in R.SECOND:
        w = case["notes"][k][0]
        assert (w == R.ROUGH).any() and ((w == R.GAVE_UP) | (w == R.NEVER)).any(), k
    w, ch, fail = case["notes"][9]
    hard = (w == R.GAVE_UP) & (ch % 4 == 3) & (fail % 4 != 3)
    assert hard.any() and set(ch[hard]) <= {3, 19}
    # the approximation changes the rough columns and no other
    for k in R.FIRST:
        rough = case["notes"][k][0] == R.ROUGH
        assert not np.array_equal(case["rough"][k][2][rough], case["exact"][k][2][rough])
        assert np.array_equal(case["rough"][k][2][~rough], case["exact"][k][2][~rough])


# ---- the flag
FULL = dict(me_nni=True, spr=2, ml_nni=20)


@pytest.mark.parametrize("flags,want", [
    ("-approxml", dict(dtype=F32, aa_model="jtt", approx_ml=True, **FULL)),
    ("-mlapprox", dict(dtype=F32, aa_model="jtt", approx_ml=True, **FULL)),
    ("-lg -double-precision -gamma -approxml", dict(dtype=F64, aa_model="lg", approx_ml=True, gamma=True, **FULL)),
    ("-wag -nome -mllen -mlapprox", dict(dtype=F32, aa_model="wag", mllen=20, approx_ml=True)),
    ("-lg -mlacc 2 -slownni -approxml", dict(dtype=F32, aa_model="lg", approx_ml=True, ml_accuracy=2, slow_nni=True, **FULL)),
    # accepted and without effect, as in the reference: nucleotides, and no ML stage
    ("-nt -approxml", dict(dtype=F32, **FULL)),
    ("-nt -nome -mllen -mlapprox", dict(dtype=F32, mllen=20)),
    ("-noml -approxml", dict(dtype=F32, aa_model="jtt", me_nni=True, spr=2)),
    ("-noml -nome -mlapprox", dict(dtype=F32, aa_model="jtt")),
    ("-mlnni 0 -approxml", dict(dtype=F32, aa_model="jtt", me_nni=True, spr=2)),
])
def test_the_flag_translates(flags, want):
    run = from_reference_flags(flags)
    assert run.kwargs == want
    assert run.other == {} and run._fields == ("n_codes", "dtype", "n_bootstrap", "kwargs", "other")
    without = from_reference_flags(" ".join(f for f in flags.split() if f not in ("-approxml", "-mlapprox")))
    assert {k: v for k, v in run.kwargs.items() if k != "approx_ml"} == without.kwargs


@pytest.mark.parametrize("flags", ["-approxml -approxml", "-mlapprox -lg -mlapprox", "-approxml -mlapprox", "-nt -mlapprox -approxml"])
def test_the_flag_given_twice_is_refused(flags):
    with pytest.raises(ValueError, match="approx"):
        from_reference_flags(flags)


# ---- nj_newick
class Recorder:
    """stands where libvft_host.so would: notes the call and fails it"""
    def __init__(self, log):
        self.log = log

    def vft_nj_ml_newick(self, *args):
        self.log.append("vft_nj_ml_newick")
        return 1


class NoDevice:
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    dt = np.dtype(np.float32)

    def __init__(self, log):
        self.log = log

    def set_approx_ml(self, on):
        self.log.append(("set_approx_ml", on))


CODES = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
NAMES = ["s%d" % k for k in range(6)]


def test_nj_newick_sets_the_switch_once_before_the_driver_runs(monkeypatch):
    def calls(**kw):
        log = []
        monkeypatch.setattr(backend, "load_host_library", lambda: Recorder(log))
        with pytest.raises(backend.VftError):
            backend.nj_newick(lambda n, L: NoDevice(log), CODES, NAMES, **kw)
        return log
    assert calls(approx_ml=True, aa_model="lg", ml_nni=20) == [("set_approx_ml", True), "vft_nj_ml_newick"]
    assert calls(**from_reference_flags("-lg -approxml").kwargs) == [("set_approx_ml", True), "vft_nj_ml_newick"]
    assert calls(aa_model="lg", ml_nni=20) == ["vft_nj_ml_newick"]                      # the default calls nothing
    assert calls(approx_ml=False, aa_model="lg", ml_nni=20) == ["vft_nj_ml_newick"]
    assert "approx_ml" not in [name for name, _ in backend._NJOptions._fields_]         # state of the context, no member of the options


# ---- the fixtures
def test_there_are_the_seven_fixtures():
    assert len(FIXTURES) == 7, FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_a_fixture_differs_from_its_control(name):
    d = G.load(name)
    flags = G.text(d["flags"]).split()
    assert "-approxml" in flags and "-nt" not in flags
    assert bytes(d["newick"]) != bytes(d["control_newick"])
    assert len(d["loglk"]) >= 1 and {"codes", "newick", "newick_support", "rates", "ratecat", "control_newick"} <= set(d)
    run = from_reference_flags(flags)
    assert run.kwargs["approx_ml"] is True and run.kwargs.get("threads", 1) == 1
    assert os.path.getsize(os.path.join(G.GOLDEN, name + ".npz")) < (1 << 20)
