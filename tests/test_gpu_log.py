"""`-log FILE` on the device: for every fixture tests/golden/log_*.npz (tools/gen_log_fixtures.py: the reference's own log of the same
command line) the lines nj_newick(..., log=...) writes are the reference's in-scope lines, in order and in number, byte for byte
behind the masked clock fields (veryfasttree_amd/stagelog.py) - every stage tree, likelihood, rate line and, with -gamma, every `%.3f`
of the per-site table.  Asking for the log does not change the tree; the stage trees do not depend on which walk path produced them;
the command-line tool writes the same file; a descriptor that cannot be written to ends the run with an error that names the log."""
import fcntl
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from veryfasttree_amd import stagelog, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(G.GOLDEN, "log_*.npz")))


def wanted(d):
    return bytes(d["log"]).decode().split("\n")


def logged_run(d, path, **more):
    from veryfasttree_amd.backend import nj_newick
    run, make, names = G.reference_run(d)
    tree = nj_newick(make, d["codes"], names, me_lengths=True, n_bootstrap=run.n_bootstrap, log=path, **dict(run.kwargs, **more))
    if path is None:
        return tree, None
    with open(path) as fh:
        return tree, fh.read()


_plain = {}


def plain_tree(name):
    """the tree of the fixture's run without a log: computed once, shared"""
    if name not in _plain:
        _plain[name] = logged_run(G.load(name), None)[0]
    return _plain[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_log_is_the_references(name, tmp_path):
    d = G.load(name)
    tree, text = logged_run(d, str(tmp_path / "run.log"))
    first, _, rest = text.partition("\n")
    assert first.startswith(stagelog.HEADER_PREFIX) and "not written" in first
    assert all(stagelog.in_scope(line) for line in rest.split("\n")[:-1]), "a line that is not in scope"
    assert text.endswith("TreeCompleted\n")
    why = stagelog.first_difference(stagelog.masked_lines(text), wanted(d))
    assert why is None, "%s: %s" % (name, why)
    assert tree == plain_tree(name), "asking for the log changed the tree"
    assert tree == G.text(d["newick"])


@pytest.mark.parametrize("flag", ["DEBUG_NO_WALK_SERVER", "DEBUG_HOST_JOINS"])
@pytest.mark.parametrize("name", FIXTURES)
def test_the_stage_trees_do_not_depend_on_the_walk_path(name, flag, tmp_path):
    """every fixture again with a launch per walk step and with the host's join loop: the same stage trees - the topology adopted in
    mid-round and the lengths downloaded behind a round do not depend on which of the equivalent loops made them"""
    from veryfasttree_amd import backend
    d = G.load(name)
    _, text = logged_run(d, str(tmp_path / "run.log"), debug_flags=getattr(backend, flag))
    trees = lambda lines: [line for line in lines if stagelog.tag(line).split("_")[0] in ("NJ", "ME", "ML")]
    why = stagelog.first_difference(trees(stagelog.masked_lines(text)), trees(wanted(d)))
    assert why is None, "%s with %s: %s" % (name, flag, why)


def test_the_tool_writes_the_same_file(tmp_path):
    d = G.load("log_nt_gtr_gamma")
    assert G.text(d["flags"]) == "-nt -gtr -gamma"
    fa, log = str(tmp_path / "in.fa"), str(tmp_path / "tool.log")
    synth.codes_to_fasta(d["codes"], fa, synth.ALPHABET_NT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "nj_tree.py"), fa, "-full", "-gtr", "-gamma", "-log", log],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    with open(log) as fh:
        text = fh.read()
    assert text.startswith(stagelog.HEADER_PREFIX)
    why = stagelog.first_difference(stagelog.masked_lines(text), wanted(d))
    assert why is None, why
    assert res.stdout.decode().strip() == G.text(d["newick"])


def test_makematrix_writes_the_first_line_alone(tmp_path):
    from veryfasttree_amd.backend import logging_to, make_matrix
    d = G.load("log_nt_gtr_gamma")
    log = str(tmp_path / "mm.log")
    with open(str(tmp_path / "matrix.txt"), "wb") as out, logging_to(log):
        make_matrix(d["codes"][:12], ["s%d" % k for k in range(12)], 4, np.float32, False, out.fileno())
    with open(log) as fh:
        text = fh.read()
    assert text.startswith(stagelog.HEADER_PREFIX) and text.count("\n") == 1


def test_a_closed_descriptor_is_an_error_that_names_the_log(tmp_path):
    """the error is write(2)'s own (EBADF): the run ends at the log's first line, before any device work of the driver.  The descriptor
    is a high number (F_DUPFD from 1000), so that nothing opened in between can take the closed number over."""
    from veryfasttree_amd.backend import VftError
    d = G.load("log_nt_mllen_nocat")
    low = os.open(str(tmp_path / "closed.log"), os.O_WRONLY | os.O_CREAT, 0o644)
    fd = fcntl.fcntl(low, fcntl.F_DUPFD, 1000)
    os.close(low)
    os.close(fd)
    with pytest.raises(VftError, match=r"-log: writing the log failed: Bad file descriptor"):
        logged_run(d, fd)
    assert (tmp_path / "closed.log").read_bytes() == b""
    assert logged_run(d, None)[0] == plain_tree("log_nt_mllen_nocat")     # logging is off again, and the next run is whole
