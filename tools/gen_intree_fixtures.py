#!/usr/bin/env python3
"""TEST INFRASTRUCTURE - regenerates tests/golden/intree_*.npz from the compiled reference (`-intree FILE`, readTree).

Authoring container only (needs oracle/_ref/VeryFastTree, `make -C oracle ref`):

    python tools/gen_intree_fixtures.py [--jobs N] [case ...]

Per case three runs of `VeryFastTree <flags> -threads T -seed 1 -intree T.nwk`:
  1. `-threads 1 -verbose 6 -noml -nome -nosupport -log`: the `Map <parse index> to <node id> (parent <parse index> nchild <k>)` lines give every
     node's id and parent, the `NJ\\t<tree>` line (all lengths 0.00000) the child order - node arrays recovered from the reference's
     own output, not from this repository's parser;
  2. the case's flags with `-nosupport -log`: the final tree, the TreeLogLk / Rates / SiteCategories lines of an ML case;
  3. the case's flags: the tree with its supports.
Start trees come from the seeded generators below or from the reference's own output on the same alignment.  Only data (inputs and
expected outputs) is written to tests/golden/; the keys follow bb_*.npz / ml_*.npz plus intree, nj_newick, parent, child, root.
"""
import os
import re

import numpy as np

import reference_run as R
from reference_run import GOLDEN, REFBIN, first_unique, rd, run, synth
from veryfasttree_amd.backend import uniquify  # noqa: E402 (reference_run puts the repository on the path)


def dups_codes():
    """60 unique rows, then two copies of row 3 (s60, s61)"""
    u = first_unique(synth.random_descent_codes(80, 60, 4, 0.10, 0.02, 91), 60)
    return np.concatenate([u, u[3:4], u[3:4]], axis=0)


def random_tree(n, seed, decorate):
    """a random rooted binary topology over s0 .. s<n-1> (a root of two); decorate: branch lengths everywhere, support labels inside"""
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = ["s%d" % k for k in rng.permutation(n)]
    while len(parts) > 1:
        i = int(rng.integers(len(parts)))
        a = parts.pop(i)
        j = int(rng.integers(len(parts)))
        b = parts.pop(j)
        if decorate:
            a += ":%.4f" % rng.random()
            b += ":%.4f" % rng.random()
            parts.append("(%s,%s)%s" % (a, b, "%.3f" % rng.random() if len(parts) else ""))
        else:
            parts.append("(%s,%s)" % (a, b))
    return parts[0] + ";\n"


def caterpillar_62(_codes):
    """a leaf first at the root, then a chain; s60 (a copy of s3) near the top, s3 itself in the middle, s61 (another copy) at the
    bottom - the first becomes the leaf, the other two are skipped and leave nodes of one child; newlines and blanks in the text"""
    order = [5, 60, 0, 1, 2] + list(range(6, 33)) + [3] + list(range(33, 60)) + [61, 4]
    assert sorted(order) == list(range(62))
    text = "s%d" % order[-1]
    for depth, k in enumerate(reversed(order[1:-1])):
        sep = " ,\n  " if depth % 7 == 0 else ", " if depth % 3 == 0 else ","
        text = "(s%d%s%s )" % (k, sep, text) if depth % 5 == 0 else "(s%d%s%s)" % (k, sep, text)
    return "( s%d ,\n%s\n) ;\n" % (order[0], text)


def reference_tree(flags):
    """the start tree is what the reference itself prints for the alignment with `flags` (a root of three, its own labels)"""
    def make(codes, tmp, name, nc):
        fa = R.write_fasta(tmp, name + "_start", codes, nc)
        return run([REFBIN] + flags + ["-threads", "1", "-seed", "1", fa]).stdout.decode()
    return make


CASES = [
    # name, flags, n_codes, threads, alignment, start tree (text, or a function of (codes, tmp, name, n_codes)), extra runs
    ("intree_nt_4", ["-nt"], 4, 1, lambda: synth.random_descent_codes(5, 40, 4, 0.2, 0.0, 27)[:4], "((s0,s1),(s2,s3));\n"),   # slow_nt_4's alignment
    ("intree_nt_5", ["-nt"], 4, 1, rd(5, 40, 4, 0.2, 0.0, 27), "((s0,s1),(s2,(s3,s4)));\n"),                                     # slow_nt_5's
    ("intree_nt_200_me", ["-nt", "-noml", "-nome"], 4, 1, rd(200, 120, 4, 0.05, 0.02, 21), random_tree(200, 101, True)),           # bb_nt_200's
    ("intree_nt_200_mllen", ["-nt", "-nome", "-mllen"], 4, 1, rd(200, 120, 4, 0.05, 0.02, 21), reference_tree(["-nt"])),
    ("intree_nt_200_full", ["-nt"], 4, 1, rd(200, 120, 4, 0.05, 0.02, 21), random_tree(200, 102, False)),
    ("intree_nt_300_double_gtr", ["-nt", "-gtr", "-double-precision"], 4, 1, rd(300, 90, 4, 0.05, 0.03, 24), reference_tree(["-nt", "-noml", "-nome"])),
    ("intree_aa_120_lg", ["-lg"], 20, 1, rd(120, 80, 20, 0.10, 0.03, 103), random_tree(120, 104, False)),
    ("intree_aa_100_wag_double_mllen", ["-wag", "-double-precision", "-nome", "-mllen"], 20, 1, rd(100, 80, 20, 0.10, 0.03, 105), random_tree(100, 106, True)),
    ("intree_nt_62_dups_caterpillar", ["-nt"], 4, 1, dups_codes, caterpillar_62),
    ("intree_nt_400_t4", ["-nt"], 4, 4, rd(400, 150, 4, 0.06, 0.02, 81), random_tree(400, 107, False)),                            # thr_full_nt_400_t4's
]
GAMMA_TOO = {"intree_nt_200_mllen"}   # the same once more with -gamma


def split_top(s):
    """the comma-separated items of a Newick group's inside"""
    out, depth, last = [], 0, 0
    for k, ch in enumerate(s):
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            out.append(s[last:k])
            last = k + 1
    return out + [s[last:]]


def nested(s):
    """'(a:1,(b:1,c:1):1)' -> nested lists of names (lengths and labels dropped)"""
    s = s.strip()
    if not s.startswith("("):
        return s.split(":")[0]
    close = s.rindex(")")
    return [nested(x) for x in split_top(s[1:close])]


def node_arrays(log_text, nj_line, aln_to_uniq, n_unique):
    """parent / child / root from the reference's Map lines (ids, parents) and its NJ line (child order)"""
    maps = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"^Map (\d+) to (-?\d+) \(parent (-?\d+) nchild \d+\)", log_text, re.M)]
    to_id = {a: b for a, b, _ in maps}
    n_nodes = max(to_id.values()) + 1
    parent = np.full(n_nodes, -1, np.int64)
    for a, b, c in maps:
        if b >= 0 and c >= 0:
            parent[b] = to_id[c]
    roots = [v for v in range(n_nodes) if parent[v] < 0]
    assert len(roots) == 1, roots
    leaves_below = [set() for _ in range(n_nodes)]
    for u in range(n_unique):
        v = u
        while v >= 0:
            leaves_below[v].add(u)
            v = parent[v]
    by_set = {frozenset(s): v for v, s in enumerate(leaves_below)}
    assert len(by_set) == n_nodes
    child = np.full((n_nodes, 3), -1, np.int64)

    def walk(t):   # -> (node id, leaf set); a group of names of ONE unique sequence is that leaf (printNJ's "(a:0.0,b:0.0)")
        if isinstance(t, str):
            u = aln_to_uniq[int(t[1:])]
            return u, frozenset([u])
        got = [walk(x) for x in t]
        allset = frozenset().union(*[g[1] for g in got])
        if len(allset) == 1:
            return got[0][0], allset
        v = by_set[allset]
        for k, g in enumerate(got):
            child[v, k] = g[0]
        return v, allset

    top, _ = walk(nested(nj_line.rstrip(";")))
    assert top == roots[0]
    return parent, child, top


def gen_case(tmp, name, flags, nc, threads, make, start):
    codes = make()
    fa = R.write_fasta(tmp, name, codes, nc)
    text = start if isinstance(start, str) else start(codes, tmp, name, nc) if start is not caterpillar_62 else start(codes)
    nwk = os.path.join(tmp, name + ".nwk")
    with open(nwk, "w") as fh:
        fh.write(text)
    model = [f for f in flags if f in ("-nt", "-lg", "-wag", "-double-precision")]
    base = ["-threads", str(threads), "-seed", "1", "-intree", nwk]
    log = os.path.join(tmp, name + ".log")
    # (the Map lines are only written at one thread; the parse and the numbering do not depend on the thread count, and the NJ line
    #  of the case's own thread count is asserted to be the same)
    run([REFBIN] + model + ["-threads", "1"] + base[2:] + ["-verbose", "6", "-noml", "-nome", "-nosupport", "-log", log, fa])
    vtext = R.read_log(log)
    nj = R.nj_line(vtext)
    if threads > 1:
        run([REFBIN] + model + base + ["-verbose", "3", "-noml", "-nome", "-nosupport", "-log", log, fa])
        assert R.nj_line(R.read_log(log)) == nj, name + ": the NJ line depends on the thread count"
    unique_first, aln_next = uniquify(codes)
    aln_to_uniq = np.full(len(codes), -1, np.int64)
    for u, k in enumerate(unique_first):
        while k >= 0:
            aln_to_uniq[k] = u
            k = aln_next[k]
    parent, child, root = node_arrays(vtext, nj, aln_to_uniq, len(unique_first))
    out = dict(codes=codes, intree=R.as_bytes(text), threads=np.int64(threads), flags=R.as_bytes(" ".join(flags)), nj_newick=R.as_bytes(nj),
               parent=parent, child=child, root=np.int64(root))
    for tag, more in [("", [])] + ([("gamma_", ["-gamma"])] if name in GAMMA_TOO else []):
        for key, v in R.one_run(tmp, name + tag, fa, flags + more, threads, nwk).items():
            out[tag + key] = v
        if more:
            m = re.search(r"Gamma\(20\) LogLk = (\S+) alpha = (\S+) rescaling lengths by (\S+)", R.read_log(os.path.join(tmp, name + tag + ".log")))
            assert m, name + ": no Gamma(20) line"
            out["gamma"] = np.array([float(m.group(k)) for k in (1, 2, 3)])
    dst = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(dst, **out)
    return "%-32s %4d rows %4d unique  %4d nodes  root %d  %7.1f KiB" % (name, len(codes), len(unique_first), len(parent), root, os.path.getsize(dst) / 1024.0)


if __name__ == "__main__":
    R.main(gen_case, CASES)
