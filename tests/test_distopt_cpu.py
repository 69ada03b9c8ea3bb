"""`-rawdist` for a tree and `-trans FILE`, everything that needs no device.

The `-trans` parser (veryfasttree_amd/host/ReadTransition.h through vft_read_aa_transition) against a numpy restatement of the reference's
checks (readAATransitionMatrix, TransitionMatrix.tcc:80-153) - on the generator's matrix, on every refusal by its message, with LF and
CRLF line ends - and as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer (host code only; nothing is loaded into
Python under a sanitizer).  The round trip: a built-in model's constants, written with %.17g and parsed, give that model's tables bit for
bit through vft_aa_tables_from_matrix.  The translation of the flags, and the driver's refusal of the "custom" model without a matrix."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
AA = "ARNDCQEGHILKMFPSTWYV"
HEADER = "\t".join(AA) + "\t*"
F32, F64 = np.float32, np.float64


def model_text(matrix, stat, fmt="%.12g", eol="\n", cell=None):
    """the file of a model; cell = {(row, column): text} replaces single fields (column 20 = the frequency)"""
    cell = cell or {}
    lines = [HEADER]
    for i in range(20):
        lines.append("\t".join([AA[i]] + [cell.get((i, j), fmt % (matrix[i, j] if j < 20 else stat[i])) for j in range(21)]))
    return eol.join(lines) + eol


def generator_model():
    from veryfasttree_amd.backend import read_aa_transition
    return read_aa_transition(bytes(G.load("trans_aa_40")["trans_text"]))


# ------------------------------------------------------------------------------------------------ the reference's checks, restated
NUMBER = re.compile(r"\s*[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?|inf(?:inity)?|nan)", re.I)


def restated(text):
    """readAATransitionMatrix on the file's text: (matrix, stat), or the message it refuses with (None: std::stod would throw)"""
    at_end = False

    def readline(state={"pos": 0}):
        nonlocal at_end
        if at_end:
            return None
        k = text.find("\n", state["pos"])
        line = text[state["pos"]:] if k < 0 else text[state["pos"]:k]
        at_end, state["pos"] = k < 0, len(text) if k < 0 else k + 1
        return line[:-1] if line.endswith("\r") else line

    def fields(line):     # std::getline(stream, field, '\t') until it fails
        out = line.split("\t")
        return out[:-1] if out[-1] == "" else out

    buf = readline()
    if buf is None:
        return "Error reading header line from transition matrix file"
    if buf != HEADER:
        return "Invalid header line in transition matrix file, it must match: " + HEADER
    matrix, stat = np.zeros((20, 20)), np.zeros(20)
    for i in range(20):
        buf = readline()
        if buf is None:
            return "Error reading matrix line"
        f = fields(buf)
        if not f or f[0] != AA[i]:
            return "Line for amino acid %c does not have the expected beginning" % AA[i]
        for j, field in enumerate(f[1:22]):      # the fields are converted as they are read: a bad one in front of a missing one wins
            m = NUMBER.match(field)
            if not m:
                return None
            if j < 20:
                matrix[i, j] = float(m.group(0))
            else:
                stat[i] = float(m.group(0))
        if len(f) < 22:
            return "Not enough fields for amino acid %c" % AA[i]
    tol = 1e-5
    tot = 0.0
    for i in range(20):
        if stat[i] < tol:
            return "stationary frequency for amino acid %c must be positive" % AA[i]
        tot += stat[i]
    if abs(tot - 1) > tol:
        return "stationary frequencies must sum to 1 -- actual sum is %g" % tot
    rate = 0.0
    for i in range(20):
        if matrix[i, i] > -tol:
            return "transition rate(%c,%c) must be negative" % (AA[i], AA[i])
        rate += stat[i] * matrix[i, i]
    if abs(rate + 1) > tol:
        return "Dot product of matrix diagonal and stationary frequencies must be -1 -- actual dot product is %g" % rate
    for j in range(20):
        col = 0.0
        for i in range(20):
            col += matrix[i, j]
            if i != j and matrix[i, j] < 0:
                return "Off-diagonal matrix entry for (%c,%c) is negative" % (AA[i], AA[j])
        if abs(col) > tol:
            return "Sum of column %c must be zero -- actual sum is %g" % (AA[j], col)
    return matrix, stat


def bad_files():
    """name -> (text, the words its refusal must hold): every refusal of the issue, one edit of the generator's matrix each"""
    m, s = generator_model()
    good = model_text(m, s)
    rows = good.split("\n")
    edit = lambda fn: model_text(*fn(m.copy(), s.copy()))

    def set_(i, j, v):
        def fn(mm, ss):
            if j < 20:
                mm[i, j] = v
            else:
                ss[i] = v
            return mm, ss
        return fn
    return {
        "header_spaces": (good.replace(HEADER, HEADER.replace("\t", " "), 1), "Invalid header line in transition matrix file, it must match: A\tR\t"),
        "header_no_star": (good.replace(HEADER, HEADER[:-2], 1), "Invalid header line"),
        "empty": ("", "Invalid header line"),
        "row_start": ("\n".join(rows[:2] + ["X" + rows[2][1:]] + rows[3:]), "Line for amino acid R does not have the expected beginning"),
        "row_start_long": ("\n".join(rows[:2] + ["R" + rows[2]] + rows[3:]), "Line for amino acid R does not have the expected beginning"),
        "few_fields": ("\n".join(rows[:3] + [rows[3].rsplit("\t", 1)[0]] + rows[4:]), "Not enough fields for amino acid N"),
        "few_fields_tab": ("\n".join(rows[:3] + [rows[3].rsplit("\t", 1)[0] + "\t"] + rows[4:]), "Not enough fields for amino acid N"),
        "ten_rows": ("\n".join(rows[:11]), "Error reading matrix line"),
        "ten_rows_newline": ("\n".join(rows[:11]) + "\n", "Line for amino acid L does not have the expected beginning"),
        "tiny_frequency": (edit(set_(3, 20, 1e-6)), "stationary frequency for amino acid D must be positive"),
        "negative_frequency": (edit(set_(19, 20, -0.05)), "stationary frequency for amino acid V must be positive"),
        "frequency_sum": (edit(lambda mm, ss: (mm, ss * 1.01)), "stationary frequencies must sum to 1 -- actual sum is 1.01"),
        "diagonal_zero": (edit(set_(2, 2, 0.0)), "transition rate(N,N) must be negative"),
        "diagonal_positive": (edit(set_(0, 0, 0.5)), "transition rate(A,A) must be negative"),
        "dot_product": (edit(lambda mm, ss: (mm * 1.1, ss)), "Dot product of matrix diagonal and stationary frequencies must be -1 -- actual dot product is -1.1"),
        "off_diagonal": (edit(set_(1, 0, -0.01)), "Off-diagonal matrix entry for (R,A) is negative"),
        "column_sum": (edit(lambda mm, ss: set_(1, 0, mm[1, 0] + 0.01)(mm, ss)), "Sum of column A must be zero -- actual sum is 0.01"),
        "not_a_number": (model_text(m, s, cell={(3, 7): "abc"}), "amino acid D"),
        "empty_field": (model_text(m, s, cell={(5, 20): " "}), "amino acid Q"),
    }


def parse_or_message(text):
    from veryfasttree_amd.backend import VftError, read_aa_transition
    try:
        return read_aa_transition(text)
    except VftError as e:
        return str(e)


def test_the_generators_matrix_parses_to_what_the_restatement_reads():
    d = G.load("trans_aa_40")
    text = bytes(d["trans_text"]).decode()
    assert "\r" not in text
    want = restated(text)
    got = parse_or_message(text)
    assert not isinstance(want, str) and not isinstance(got, str), (want, got)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(bytes(G.load("trans_aa_12x2200")["trans_text"]), bytes(d["trans_text"]))   # one model for both files
    # the generator's own statement of it: reversible, normalised, columns summing to zero
    import gen_distopt_fixtures as gen
    m, s = gen.random_model()
    assert gen.model_text(m, s) == bytes(d["trans_text"])
    assert np.allclose(got[0], m, rtol=1e-11, atol=1e-13) and np.allclose(got[1], s, rtol=1e-11)
    assert np.allclose(m * s[None, :], (m * s[None, :]).T, rtol=1e-12) and abs((s * np.diag(m)).sum() + 1) < 1e-12


@pytest.mark.parametrize("eol", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_line_ends_and_what_follows_the_table_are_not_read(eol):
    m, s = generator_model()
    plain = parse_or_message(model_text(m, s))
    for text in (model_text(m, s, eol=eol), model_text(m, s, eol=eol) + "anything" + eol + "at all",
                 model_text(m, s, eol=eol)[:-len(eol)],                                  # no line end behind the last row
                 model_text(m, s, eol="\textra" + eol).replace(HEADER + "\textra", HEADER, 1)):   # a 23rd field in every row
        got = parse_or_message(text)
        assert not isinstance(got, str), got
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
        want = restated(text)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # std::stod: blanks in front and a tail that is no number
    got = parse_or_message(model_text(m, s, cell={(4, 4): " %.12gxyz" % m[4, 4]}))
    assert np.array_equal(got[0], plain[0])


@pytest.mark.parametrize("name", sorted(["header_spaces", "header_no_star", "empty", "row_start", "row_start_long", "few_fields", "few_fields_tab", "ten_rows",
                                         "ten_rows_newline", "tiny_frequency", "negative_frequency", "frequency_sum", "diagonal_zero", "diagonal_positive",
                                         "dot_product", "off_diagonal", "column_sum", "not_a_number", "empty_field"]))
def test_every_refusal_is_the_references(name):
    text, words = bad_files()[name]
    got, want = parse_or_message(text), restated(text)
    assert isinstance(got, str) and words in got, got
    if want is None:     # the reference lets std::stod throw: here an error that names the amino acid
        assert "is not a number" in got
    else:
        assert got == want


def test_the_refusals_cover_the_list():
    assert len(bad_files()) == 19


@pytest.mark.parametrize("sanitize", [False, True])
def test_parser_as_a_stand_alone_program(tmp_path, sanitize):
    exe = str(tmp_path / "rtcheck")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++11", "-Wall"] + flags + [os.path.join(ROOT, "tests", "native", "read_transition_check.cpp"), "-o", exe], check=True)
    m, s = generator_model()
    files = dict(bad_files(), good=(model_text(m, s), None), good_crlf=(model_text(m, s, eol="\r\n"), None), good_no_end=(model_text(m, s)[:-1], None),
                 header_only=(HEADER, "Error reading matrix line"))
    for name, (text, _) in files.items():
        (tmp_path / name).write_bytes(text.encode())
    res = subprocess.run([exe] + [str(tmp_path / name) for name in files], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0 and out.strip().endswith("unread 0"), out[-3000:]
    for name, (text, words) in files.items():
        line = re.search(r"^file %s (.*)$" % name, out, re.M).group(1)
        if words is None:
            assert line.startswith("ok "), line
            assert abs(float(line.split()[1]) - m.sum()) < 1e-9 and abs(float(line.split()[2]) - 1) < 1e-9
        else:
            want = restated(text)
            assert line.startswith("refused (") and words in line, line
            assert want is None or line == "refused (%s)" % want


# ------------------------------------------------------------------------------------------------ the round trip
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("model", ["wag", "jtt", "lg"])
def test_a_built_in_models_file_gives_its_tables_bit_for_bit(model, dtype):
    from veryfasttree_amd import backend
    matrix, stat = backend.aa_model_matrix(model)
    assert matrix.shape == (20, 20) and (np.diag(matrix) < 0).all() and abs(stat.sum() - 1) < 1e-5
    m2, s2 = backend.read_aa_transition(model_text(matrix, stat, fmt="%.17g"))
    assert m2.tobytes() == matrix.tobytes() and s2.tobytes() == stat.tobytes()
    got, want = backend.aa_tables_from_matrix(m2, s2, dtype), backend.aa_model_tables(model, dtype)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    got, want = backend.aa_near_tables_from_matrix(m2, s2, dtype), backend.aa_near_tables(model, dtype)
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
    # and the model that was set is the model the driver builds for aa_model = "custom"
    with backend.aa_transition((m2, s2)):
        assert backend.load_host_library().vft_nj_get_aa_transition() == 1
        custom = backend.aa_model_tables("custom", dtype)
    assert backend.load_host_library().vft_nj_get_aa_transition() == 0
    for key, v in backend.aa_model_tables(model, dtype).items():
        assert custom[key].tobytes() == v.tobytes(), key


def test_another_matrix_gives_other_tables():
    from veryfasttree_amd import backend
    m, s = generator_model()
    got = backend.aa_tables_from_matrix(m, s, F64)
    assert np.array_equal(got["stat"], s) and np.allclose(got["statinv"], 1 / s, rtol=1e-15)
    # eigen-decomposition of the rate matrix: V diag(eigenval) V^-1 = M with V = codefreq^T rows ... checked as M V = V L
    V = got["codefreq"][:20]                 # codefreq[i][k] = component k of state i: the columns of V are right eigenvectors
    assert np.allclose(m @ V, V * got["eigenval"][None, :], atol=1e-10)
    assert np.allclose(got["eigeninv"] @ V, np.eye(20), atol=1e-10)
    assert not np.allclose(got["eigenval"], backend.aa_model_tables("jtt", F64)["eigenval"])


# ------------------------------------------------------------------------------------------------ the flags
def test_refflags_keeps_both_options_for_the_caller():
    from veryfasttree_amd.refflags import from_reference_flags
    plain = from_reference_flags("-wag")
    run = from_reference_flags("-wag -trans model.txt")
    assert run.other == dict(trans="model.txt") and run.kwargs == plain.kwargs and run.n_codes == 20       # (no file is opened)
    assert from_reference_flags(["-trans", "a file.txt", "-noml"]).other == dict(trans="a file.txt")
    for flags in ("-nt -trans model.txt", "-trans model.txt -nt -noml"):
        with pytest.raises(ValueError, match="-trans"):
            from_reference_flags(flags)
    with pytest.raises(ValueError, match="-trans"):
        from_reference_flags("-trans")
    with pytest.raises(ValueError, match="-trans"):
        from_reference_flags("-trans a -trans b")
    for flags in ("-nt", "-nt -noml", "-nt -noml -nome", "", "-lg -double-precision", "-nt -noml -pseudo"):
        raw, ctl = from_reference_flags(flags + " -rawdist"), from_reference_flags(flags)
        assert raw.kwargs == ctl.kwargs and raw.other == dict(rawdist=True) and ctl.other == {}
        assert (raw.n_codes, raw.dtype, raw.n_bootstrap) == (ctl.n_codes, ctl.dtype, ctl.n_bootstrap)


def test_every_new_fixture_records_its_control_and_its_option():
    import glob
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G.GOLDEN, "*.npz")) if re.match(r"(rawdist|trans)_", os.path.basename(p)))
    assert names == ["rawdist_aa_40", "rawdist_nt_16x1707", "rawdist_nt_60", "trans_aa_12x2200", "trans_aa_40"]
    from veryfasttree_amd.refflags import from_reference_flags
    for name in names:
        d = G.load(name)
        option = "rawdist" if name.startswith("rawdist") else "trans"
        assert ("trans_text" in d) == (option == "trans")
        for k in range(int(d["n_runs"])):
            pre = "r%d_" % k
            run = from_reference_flags(G.text(d[pre + "flags"]), threads=int(d[pre + "threads"]), intree_text="(a,b,(c,d));" if pre + "intree" in d else None)
            assert option in run.other
            assert bytes(d[pre + "newick"]) != bytes(d[pre + "control_newick"])
            assert bytes(d[pre + "newick_support"]) != bytes(d[pre + "control_newick_support"])
            assert (pre + "loglk" in d) == (pre + "control_loglk" in d) == ("-noml" not in G.text(d[pre + "flags"]).split())


# ------------------------------------------------------------------------------------------------ the driver, before the device
class NoDevice:
    ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    dt = np.dtype(np.float32)
    n_codes = 20

    def set_raw_distances(self, on):
        self.raw = on


def newick_without_a_device(**kw):
    from veryfasttree_amd import backend
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    return backend.nj_newick(lambda n, L: NoDevice(), codes, ["s%d" % k for k in range(6)], me_lengths=True, **kw)


def test_the_driver_refuses_the_custom_model_without_a_matrix_before_the_device():
    from veryfasttree_amd import backend
    backend.set_aa_transition(None)
    for kw in (dict(ml_nni=20, me_nni=True, spr=2), dict(mllen=20), dict()):
        with pytest.raises(backend.VftError, match=r"vft_nj_options\.aa_model = 4 \(-trans\) without a matrix: vft_nj_set_aa_transition comes first"):
            newick_without_a_device(aa_model="custom", **kw)
    assert backend.AA_MODELS["custom"] == 4
    # the tables of the custom model without one: an error, not JTT's
    with pytest.raises(backend.VftError):
        backend.aa_model_tables("custom")
    # what is set must be usable: frequencies positive, everything finite - and a refused call sets nothing
    m, s = generator_model()
    for bad in ((m, np.where(np.arange(20) == 3, 0.0, s)), (np.where(np.eye(20) > 0, np.nan, m), s), (m[:19], s)):
        with pytest.raises(backend.VftError):
            backend.set_aa_transition(bad)
        assert backend.load_host_library().vft_nj_get_aa_transition() == 0
    # a bad file given to nj_newick is refused with the parser's message, and leaves nothing set
    with pytest.raises(backend.VftError, match="Invalid header line"):
        newick_without_a_device(aa_trans="not a matrix\n", mllen=20)
    assert backend.load_host_library().vft_nj_get_aa_transition() == 0


def test_trans_on_nucleotides_is_refused_by_nj_newick():
    from veryfasttree_amd import backend
    m, s = generator_model()

    class Nucleotides(NoDevice):
        n_codes = 4
    codes = np.array([[(k >> (2 * p)) & 3 for p in range(12)] for k in range(6)], np.uint8)
    with pytest.raises(backend.VftError, match="-trans"):
        backend.nj_newick(lambda n, L: Nucleotides(), codes, ["s%d" % k for k in range(6)], me_lengths=True, mllen=20, aa_trans=(m, s))
    assert backend.load_host_library().vft_nj_get_aa_transition() == 0
