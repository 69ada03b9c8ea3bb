"""`-log FILE` without a device: which lines are in scope and how their clocks are masked (veryfasttree_amd/stagelog.py), the
translation of the flag, what the fixtures tests/golden/log_*.npz hold (tools/gen_log_fixtures.py), and the switch of the C ABI
(vft_nj_set_log) on runs that end before anything reaches a context."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import golden_util as G
from veryfasttree_amd import stagelog
from veryfasttree_amd.refflags import from_reference_flags

FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G.GOLDEN, "log_*.npz")))


def lines_of(d):
    return bytes(d["log"]).decode().split("\n")


# ------------------------------------------------------------------------------------------------ masking
@pytest.mark.parametrize("line,masked", [
    ("Initial topology in 0.03 seconds", "Initial topology in # seconds"),
    ("Total branch-length 2.802 after 12.41 sec", "Total branch-length 2.802 after # sec"),
    ("2 rounds ML lengths: LogLk = -2295.621 Max-change 0.0006 (converged) Time 0.07", "2 rounds ML lengths: LogLk = -2295.621 Max-change 0.0006 (converged) Time #"),
    ("1 rounds ML lengths: LogLk ~= -2295.622 Max-change 0.0167 Time 100.50", "1 rounds ML lengths: LogLk ~= -2295.622 Max-change 0.0167 Time #"),
    ("ML-NNI round 1: LogLk = -2034.466 NNIs 10 max delta 2.25 Time 0.04", "ML-NNI round 1: LogLk = -2034.466 NNIs 10 max delta 2.25 Time #"),
    ("ML-NNI round 4: LogLk ~= -1978.774 NNIs 0 max delta 0.00 Time 0.10 (final)", "ML-NNI round 4: LogLk ~= -1978.774 NNIs 0 max delta 0.00 Time # (final)"),
    ("Optimize all lengths: LogLk = -1978.762 Time 0.10", "Optimize all lengths: LogLk = -1978.762 Time #"),
    ("Total time: 0.13 seconds Unique: 40/42 Bad splits: 0/37", "Total time: # seconds Unique: 40/42 Bad splits: 0/37"),
    ("Total time: 3.50 seconds Unique: 64/64 Bad splits: 7/61 Worst delta-LogLk 2.017", "Total time: # seconds Unique: 64/64 Bad splits: 7/61 Worst delta-LogLk 2.017")])
def test_the_clock_of_every_clock_bearing_line_is_masked(line, masked):
    assert stagelog.in_scope(line)
    assert stagelog.mask(line) == masked
    assert stagelog.mask(masked) == masked


@pytest.mark.parametrize("line", [
    "Refining topology: 21 rounds ME-NNIs, 2 rounds ME-SPRs, 11 rounds ML-NNIs", "Turning off heuristics for final round of ML NNIs (converged)",
    "Gamma(20) LogLk = -2035.282 alpha = 9.982 rescaling lengths by 0.997", "TreeLogLk\tML_NNI1\t-2034.4658\tMaxChange\t2.2526",
    "Gamma20\t7\t-4.210\t-1.770", "NJ\t(a:0.10000,b:0.20000,c:0.30000);", "NNI: 10 SPR: 0 ML-NNI: 13", "TreeCompleted"])
def test_a_line_without_a_clock_stays_as_it_is(line):
    assert stagelog.in_scope(line) and stagelog.mask(line) == line


@pytest.mark.parametrize("line", [
    "Command: VeryFastTree -nt -log x in.fa", "VeryFastTree Version 4.0.5 (OpenMP, AVX2) with SSE3", "Alignment: in.fa", "Read 42 sequences, 150 positions",
    "Nucleotide distances: Jukes-Cantor Joins: balanced Support: SH-like 1000", "TopHits: 1.00*sqrtN close=default refresh=0.80",
    "Dist/N**2: by-profile 6.399 (out 0.421) by-leaf 0.614 avg-prof 4.216", "Top hits: close neighbors 29/40 2nd-level 0 refreshes 10 Hill-climb: 0 Update-best: 5",
    "Max-lk operations: lk 30249 posterior 10293 star-only 57", "Use -gamma for approximate but comparable Gamma(20) log-likelihoods",
    stagelog.HEADER_PREFIX + " anything", ""])
def test_what_is_out_of_scope(line):
    assert not stagelog.in_scope(line)


def test_a_difference_is_named_by_its_tag():
    a = ["NJ\t(a,b);", "ME_SPR1\t(a,b);", "TreeLogLk\tML_NNI2\t-1.0\tMaxChange\t0.1", "TreeCompleted"]
    assert stagelog.first_difference(a, list(a)) is None
    assert "ME_SPR1" in stagelog.first_difference([a[0], "ME_SPR1\t(b,a);"] + a[2:], a)
    assert "TreeLogLk ML_NNI2" in stagelog.first_difference(a[:2] + ["TreeLogLk\tML_NNI2\t-1.1\tMaxChange\t0.1", a[3]], a)
    assert "TreeCompleted" in stagelog.first_difference(a[:3], a)          # the counts are compared too
    assert "TreeCompleted" in stagelog.first_difference(a + ["TreeCompleted"], a)


# ------------------------------------------------------------------------------------------------ the flag
def test_log_takes_a_file_name_and_goes_to_other():
    run = from_reference_flags("-nt -gamma -log run.log")
    assert run.other == {"log": "run.log"}
    assert run.kwargs == from_reference_flags("-nt -gamma").kwargs          # additive: nothing else moves
    assert from_reference_flags(["-log", "a b.log", "-lg"]).other == {"log": "a b.log"}
    assert "log" not in from_reference_flags("-nt").other


@pytest.mark.parametrize("flags", ["-nt -log", "-nt -log a.log -log b.log"])
def test_a_missing_name_and_a_second_log_are_value_errors_that_name_the_flag(flags):
    with pytest.raises(ValueError, match="-log"):
        from_reference_flags(flags)


def test_the_tool_hands_the_file_name_on():
    import importlib.util
    spec = importlib.util.spec_from_file_location("nj_tree_for_log", os.path.join(os.path.dirname(G.GOLDEN), os.pardir, "tools", "nj_tree.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    _, run, _ = tool.translate(["in.fa", "-full", "-gamma", "-log", "x.log"])
    assert run.other == {"log": "x.log"} and run.kwargs["gamma"] is True
    with pytest.raises(SystemExit, match="-log"):
        tool.translate(["in.fa", "-log"])


# ------------------------------------------------------------------------------------------------ the fixtures
def test_there_are_the_cases_the_log_is_pinned_on():
    assert len(FIXTURES) >= 12
    flags = {name: G.text(G.load(name)["flags"]) for name in FIXTURES}
    for wanted in ("-nt", "-nt -gtr -gamma", "-nt -double-precision -gtr", "-nt -noml", "-nt -noml -nome", "-nt -nome -mllen -nocat", "-nt -nome -mllen -cat 5",
                   "-lg -gamma", "-wag -double-precision", "-approxml", "-nt -spr 4 -mlacc 2 -slownni", "-nt -slow -nome -mllen", "-nt -pseudo"):
        assert wanted in flags.values(), wanted
    assert any(int(G.load(name)["threads"]) > 1 for name in FIXTURES)
    assert any("intree" in G.load(name) for name in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_a_fixture_holds_in_scope_lines_only(name):
    d = G.load(name)
    lines = lines_of(d)
    assert all(stagelog.in_scope(line) for line in lines)
    assert [stagelog.mask(line) for line in lines] == lines                 # stored masked
    assert not any(re.match(r"Command:|VeryFastTree Version|Dist/N\*\*2|Top hits:|Max-lk operations:", line) for line in lines)
    assert sum(line.startswith("NJ\t") for line in lines) == 1 and lines[0].startswith("NJ\t")
    assert lines.count("TreeCompleted") == 1 and lines[-1] == "TreeCompleted"
    from_reference_flags(G.text(d["flags"]), threads=int(d["threads"]), intree_text=bytes(d["intree"]).decode() if "intree" in d else None)
    # the summary block of counts is a one-thread matter (VeryFastTreeImpl.tcc:425-450)
    if int(d["threads"]) > 1:
        assert not any(line.startswith("NNI: ") for line in lines)


def test_one_fixture_has_duplicate_sequences():
    seen = []
    for name in FIXTURES:
        m = [re.search(r"Unique: (\d+)/(\d+) ", line) for line in lines_of(G.load(name)) if line.startswith("Total time: ")]
        assert len(m) == 1 and m[0]
        seen.append((int(m[0].group(1)), int(m[0].group(2))))
        assert seen[-1][1] == len(G.load(name)["codes"])
    assert any(u < n for u, n in seen)


@pytest.mark.parametrize("name", [n for n in FIXTURES if "-gamma" in G.text(G.load(n)["flags"]).split()])
def test_a_gamma_fixture_holds_one_table_row_per_site(name):
    d = G.load(name)
    n_pos = d["codes"].shape[1]
    lines = lines_of(d)
    m = re.search(r"-cat (\d+)", G.text(d["flags"]))
    n_cat = int(m.group(1)) if m else 20
    tagged = [line for line in lines if line.startswith("Gamma%d\t" % n_cat)]
    header, rows = tagged[0], tagged[1:]
    assert header.split("\t")[:3] == ["Gamma%d" % n_cat, "Site", "LogLk"] and len(header.split("\t")) == n_cat + 3
    assert len(rows) == n_pos
    for k, row in enumerate(rows):
        fields = row.split("\t")
        assert len(fields) == n_cat + 3 and fields[1] == str(k)
        assert all(re.fullmatch(r"-?\d+\.\d{3}", f) for f in fields[2:])
    assert sum(line.startswith("Gamma%dLogLk\t" % n_cat) for line in lines) == 1


def test_there_is_a_gamma_fixture():
    assert sum("-gamma" in G.text(G.load(n)["flags"]).split() for n in FIXTURES) >= 2


# ------------------------------------------------------------------------------------------------ the switch of the C ABI
class NoDevice:
    """stands where a context would: the refusals below come before anything looks at it"""
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)


def refused_run(**kw):
    from veryfasttree_amd import backend
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    with pytest.raises(backend.VftError, match="-pseudo takes a finite weight >= 0"):
        backend.nj_newick(lambda n, L: NoDevice(), codes, ["s%d" % k for k in range(6)], me_lengths=True, pseudo=-1.0, **kw)


def test_the_switch_goes_on_and_off(tmp_path):
    """vft_nj_set_log / vft_nj_get_log: the state itself.  Without a device no run gets as far as the log's first line, so that a
    descriptor switched off is not written to is shown by the state here and by a whole run on the device (tests/test_gpu_log.py)."""
    from veryfasttree_amd import backend
    assert backend.get_log() == -1                      # off is the default
    path = tmp_path / "off.log"
    fd = os.open(str(path), os.O_WRONLY | os.O_CREAT, 0o644)
    try:
        backend.set_log(fd)
        assert backend.get_log() == fd
        backend.set_log(-1)
        assert backend.get_log() == -1
        backend.set_log(fd)
        backend.set_log(-7)                             # any negative descriptor is "off"
        assert backend.get_log() == -1
        backend.set_log(fd)
        backend.set_log(None)
        assert backend.get_log() == -1
        with backend.logging_to(np.int64(fd)):          # an integer of any type is a descriptor, and stays the caller's
            assert backend.get_log() == fd
        assert backend.get_log() == -1
        with pytest.raises(RuntimeError, match="inside"):
            with backend.logging_to(fd):
                raise RuntimeError("inside")
        assert backend.get_log() == -1                  # off again behind an error
        refused_run()
        assert os.fstat(fd).st_size == 0 and os.lseek(fd, 0, os.SEEK_CUR) == 0
    finally:
        backend.set_log(-1)
        os.close(fd)
    assert path.read_bytes() == b""


def test_a_refused_run_writes_nothing_and_leaves_logging_off(tmp_path):
    from veryfasttree_amd import backend
    path = tmp_path / "refused.log"
    refused_run(log=str(path))
    assert path.read_bytes() == b""                     # created, and the refusal came before the first line
    assert backend.get_log() == -1
    refused_run(log=None)                               # and the descriptor, closed by now, is not written to again
    # a start tree that does not parse is refused before the log opens, too
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    with pytest.raises(backend.VftError):
        backend.nj_newick(lambda n, L: NoDevice(), codes, ["s%d" % k for k in range(6)], me_lengths=True, intree="((s0,s1),(s2,(s3,s4", log=str(path))
    assert path.read_bytes() == b"" and backend.get_log() == -1
    with pytest.raises(OSError):
        refused_run(log=str(tmp_path / "no such directory" / "x.log"))


def test_the_switch_is_declared_as_process_state():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "vft_host.h")).read()
    assert re.search(r"^int vft_nj_set_log\(int32_t fd\);", text, re.M)
    body = text[text.index("typedef struct {\n    int32_t fastest;"):text.index("} vft_nj_options;")]
    assert "log" not in re.findall(r"^    (?:const )?\w+ \*?(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)
