"""TEST INFRASTRUCTURE - what the fixture generators (tools/gen_*_fixtures.py) share: how they call the compiled reference
(oracle/_ref/VeryFastTree, `make -C oracle ref`; authoring container only) and what they read out of its output."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veryfasttree_amd import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
REFBIN = os.path.join(ROOT, "oracle", "_ref", "VeryFastTree")
TIME_LIMIT = 600   # seconds; a run takes seconds to a few minutes, and the reference can spin for ever


def run(cmd):
    env = dict(os.environ, OMP_WAIT_POLICY="passive")
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=TIME_LIMIT)


def rd(n, L, nc, mu, gap, seed):
    return lambda: synth.random_descent_codes(n, L, nc, mu, gap, seed)


def first_unique(codes, k):
    """the first k distinct rows, in first-occurrence order"""
    seen, rows = set(), []
    for row in codes:
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            rows.append(row)
        if len(rows) == k:
            return np.stack(rows)
    raise AssertionError("fewer than %d unique rows" % k)


def write_fasta(tmp, name, codes, nc):
    fa = os.path.join(tmp, name + ".fa")
    synth.codes_to_fasta(codes, fa, synth.ALPHABET_AA if nc == 20 else synth.ALPHABET_NT)
    return fa


def as_bytes(text):
    return np.frombuffer(text if isinstance(text, bytes) else text.encode(), dtype=np.uint8)


def read_log(log):
    return open(log, errors="replace").read()


def nj_line(text, what="NJ"):
    """the tree of the log's `NJ\\t<tree>` line (or its `ME_Lengths` line)"""
    m = re.search(r"^%s\t(\(.*;)\s*$" % what, text, re.M)
    assert m, "no %s tree line" % what
    return m.group(1)


def ml_log_lines(text, tag):
    """loglk (every TreeLogLk line), rates and ratecat (0-based) of an ML run's log"""
    ll = [float(m.group(1)) for m in re.finditer(r"^TreeLogLk\t\S+\t(\S+)", text, re.M)]
    assert ll, "no TreeLogLk lines for " + tag
    return dict(loglk=np.array(ll), rates=np.array([float(x) for x in re.search(r"^Rates((?: \S+)+)$", text, re.M).group(1).split()]),
                ratecat=np.array([int(x) - 1 for x in re.search(r"^SiteCategories((?: \d+)+)$", text, re.M).group(1).split()], dtype=np.int32))


def strip_lengths(t):
    return re.sub(rb"\)[0-9.]+:", b"):", re.sub(rb":[0-9.eE+-]+", b":", bytes(t)))


def one_run(tmp, tag, fa, flags, threads, intree=None):
    """`VeryFastTree <flags> -threads T -seed 1 [-intree FILE]`: newick (with -nosupport), newick_support, and of a run with an ML stage
    loglk / rates / ratecat.  At more than one thread two runs must print the same bytes, and the `NJ` log line must be the
    one-thread run's (no NJ phase with -intree)."""
    at = lambda t: [REFBIN] + flags + ["-threads", str(t), "-seed", "1"] + (["-intree", intree] if intree else [])
    cmd = at(threads)
    log = os.path.join(tmp, tag + ".log")
    res = run(cmd + ["-nosupport", "-log", log, fa])
    res2 = run(cmd + [fa])
    out = dict(newick=as_bytes(res.stdout), newick_support=as_bytes(res2.stdout))
    if threads > 1:
        assert run(cmd + [fa]).stdout == res2.stdout, tag + ": two runs at %d threads print different trees" % threads
        if not intree:
            log1 = os.path.join(tmp, tag + "_t1.log")
            run(at(1) + ["-nosupport", "-log", log1, fa])
            assert nj_line(read_log(log)) == nj_line(read_log(log1)), tag + ": the NJ line depends on the thread count"
    if "-noml" not in flags:
        out.update(ml_log_lines(read_log(log), tag))
    return out


def main(gen, cases):
    """`[--jobs N] [name ...]`: gen(tmp, *case) for every case whose first entry is named (all of them without names), N at a time;
    prints what each returns"""
    args = sys.argv[1:]
    jobs = 4
    if "--jobs" in args:
        k = args.index("--jobs")
        jobs = int(args[k + 1])
        del args[k:k + 2]
    assert os.path.exists(REFBIN), "build the reference first: make -C oracle ref"
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(jobs) as pool:
        for f in [pool.submit(gen, tmp, *c) for c in cases if not args or c[0] in args]:
            print(f.result(), flush=True)
