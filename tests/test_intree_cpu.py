"""`-intree`, the host half (veryfasttree_amd/host/ReadTree.h through vft_read_tree): the reference's tokenizer, parse, tree simplification and
node numbering (NJ.tcc:2449-2665) restated without a device.  The expected node arrays of the fixtures were recovered from the reference's own
`-verbose 6` log (tools/gen_intree_fixtures.py: its `Map` lines and its `NJ` line), not from this parser."""
import time

import numpy as np
import pytest

import golden_util as G

FIXTURES = ["intree_nt_4", "intree_nt_5", "intree_nt_200_me", "intree_nt_200_mllen", "intree_nt_200_full", "intree_nt_300_double_gtr",
            "intree_aa_120_lg", "intree_aa_100_wag_double_mllen", "intree_nt_62_dups_caterpillar", "intree_nt_400_t4"]


def distinct_codes(n, L=12):
    """n different rows (row k spells k in base 4)"""
    return np.array([[(k >> (2 * p)) & 3 for p in range(L)] for k in range(n)], np.uint8)


def parse(text, n=4, dup_of=(), **kw):
    """names a, b, c, ...; dup_of: {row: the earlier row it repeats}"""
    from veryfasttree_amd.backend import read_tree
    codes = distinct_codes(n)
    for k, src in dict(dup_of).items():
        codes[k] = codes[src]
    return read_tree(text, [chr(ord("a") + k) for k in range(n)], codes, **kw)


@pytest.mark.parametrize("name", FIXTURES)
def test_node_arrays_are_the_references(name):
    from veryfasttree_amd.backend import read_tree
    d = G.load(name)
    codes = d["codes"]
    parent, child, root = read_tree(bytes(d["intree"]).decode(), ["s%d" % k for k in range(len(codes))], codes)
    n = len(np.unique(codes, axis=0))
    assert root == int(d["root"]) == n                # the root is the FIRST internal id, not the last as after fastNJ
    assert len(parent) == 2 * n - 2
    assert np.array_equal(parent, d["parent"])
    assert np.array_equal(child, d["child"])          # child order is list order: it decides what printNJ prints first


def test_fixture_with_duplicates_really_skips_and_simplifies():
    """s60 and s61 repeat s3: the first of the three in the text (s60) places the leaf, the other two leave nodes of one child behind"""
    from veryfasttree_amd.backend import read_tree, uniquify
    d = G.load("intree_nt_62_dups_caterpillar")
    unique_first, aln_next = uniquify(d["codes"])
    assert len(unique_first) == 60 and aln_next[3] == 60 and aln_next[60] == 61
    text = bytes(d["intree"]).decode()
    assert "\n" in text and " " in text and text.index("s60") < text.index("s3 ") < text.index("s61")
    parent, child, root = read_tree(text, ["s%d" % k for k in range(62)], d["codes"])
    # "( s5 , (s60, (s0, ..." : a leaf first at the root; the root of two dissolves its other child, so unique sequence 3 - standing
    # where s60 stood - and the rest of the chain come up beside s5
    assert list(child[root]) == [5, 3, root + 1] and list(child[root + 1][:2]) == [0, root + 2]


@pytest.mark.parametrize("text,what", [
    ("a;", "Tree parse error: unexpected token 'a' -- No '(' at start"),
    ("", "Tree parse error: unexpected token '(End of file)' -- No '(' at start"),
    ("((),a,b,c);", "Tree parse error: unexpected token ')' -- while reading parentheses"),
    ("((a,b);", "Tree parse error: unexpected token ';' -- unbalanced parentheses"),
    ("((a,b)(c,d));", "Tree parse error: unexpected token '(' -- unexpected '(' after ')'"),
    ("((a:x,b),(c,d));", "Tree parse error: unexpected token 'x' -- not recognized as a branch length"),
    ("((a,b),(c,d):", "Tree parse error: unexpected token '(End of file)' -- not recognized as a branch length"),
    ("(a,b)),(c,d));", "Tree parse error: unexpected token ',' -- too many ')'"),
    ("(a,b;c,d);", "Tree parse error: unexpected token ';' -- unexpected token"),
    ("((a,b),(c,sX));", "Tree parse error: unexpected token 'sX' -- not recognized as a sequence name"),
    ("((a,b),('c',d));", "Tree parse error: unexpected token ''c'' -- not recognized as a sequence name"),   # no quoting
])
def test_parse_errors_carry_the_references_text(text, what):
    from veryfasttree_amd.backend import VftError
    with pytest.raises(VftError) as e:
        parse(text)
    assert str(e.value) == what


def test_a_missing_sequence_is_the_references_two_line_error():
    from veryfasttree_amd.backend import VftError
    with pytest.raises(VftError) as e:
        parse("((a,b),(c,d));", n=5)
    assert str(e.value) == ("Alignment sequence 4 (unique 4) absent from input tree\n"
                            "The starting tree (the argument to -intree) must include all sequences in the alignment!")
    with pytest.raises(VftError) as e:   # row c repeats row a: the unique sequences are a b d e f, and d - row 3, unique 2 - is the first one missing
        parse("((a,b),(c,f));", n=6, dup_of={2: 0})
    assert str(e.value).startswith("Alignment sequence 3 (unique 2) absent from input tree\n")


@pytest.mark.parametrize("text,n,leaf", [
    ("((a,b,c),d,(e,f));", 6, "a"),        # a trifurcation below the root
    ("(a,b,c,d);", 4, "a"),                # a root of four
    ("((a,b),c,d,e);", 5, "a"),            # a root of four whose first child is a node
    ("(f,(b,c,d,e),a);", 6, "b"),          # four children below the root
    ("((a,b,c),(d,e));", 5, "a"),          # the root of two dissolves (d,e); (a,b,c) stays a trifurcation
])
def test_polytomies_are_refused_not_undefined(text, n, leaf):
    """the reference only asserts (nChild < 3), compiled out of its release build: it writes past child[3]"""
    from veryfasttree_amd.backend import VftError
    with pytest.raises(VftError) as e:
        parse(text, n=n)
    assert "must be binary" in str(e.value) and "first leaf is '%s'" % leaf in str(e.value)


def test_a_leaf_only_text_is_refused():
    from veryfasttree_amd.backend import VftError
    for text in ("a;", "a", "a,b,c,d;"):
        with pytest.raises(VftError):
            parse(text)


def test_a_subtree_of_skipped_duplicates_disappears_without_trace():
    """rows a b c d e f with e = a and f = b: (e,f) holds nothing new; ((e,f),c) is then a node of one child and goes too, c moving to the
    END of the root's list (readTreeRemove); the result is the tree of ((a,b),d,c)"""
    with_dups = parse("((a,b),((e,f),c),d);", n=6, dup_of={4: 0, 5: 1})
    plain = parse("((a,b),d,c);", n=4)
    for x, y in zip(with_dups, plain):
        assert np.array_equal(x, y)
    parent, child, root = with_dups
    assert root == 4 and list(child[4]) == [5, 3, 2] and list(child[5]) == [0, 1, -1] and list(parent) == [5, 5, 4, 4, -1, 4]
    # another name of a sequence seen before, and the same name twice, are skipped alike
    assert np.array_equal(parse("((a,b),(c,(d,a)));")[1], parse("((a,b),(c,d));")[1])
    assert np.array_equal(parse("((e,c),(d,(a,b)));", n=6, dup_of={4: 0, 5: 1})[1][4:], [[5, 0, 2], [3, 1, -1]])


def test_a_label_that_is_no_number_warns_and_parses():
    got = parse(" ( ( a:0.1 ,b:2e-3)0.95:0.1,\n c ,\t(d:1,e:-0.5)lab:3 ) ;", n=5, return_warnings=True)
    parent, child, root, warnings = got
    assert warnings == ["Warning while parsing tree: non-numeric label lab for internal node"]
    plain = parse("((a,b),c,(d,e));", n=5, return_warnings=True)
    assert plain[3] == [] and np.array_equal(parent, plain[0]) and np.array_equal(child, plain[1])
    assert root == 5 and list(child[5]) == [7, 2, 6]   # the stack pops the LAST child first: (d,e) is node 6, (a,b) node 7


def test_a_caterpillar_of_200000_leaves():
    """no recursion anywhere (a Python or C stack of 200 000 frames would not survive) and linear time"""
    from veryfasttree_amd.backend import read_tree
    n = 200000
    names = ["t%d" % k for k in range(n)]
    text = "".join("(t%d," % k for k in range(n - 1)) + "t%d" % (n - 1) + ")" * (n - 1) + ";"
    unique = (np.arange(n, dtype=np.int64), np.full(n, -1, np.int64))   # every row its own sequence
    t0 = time.perf_counter()
    parent, child, root = read_tree(text, names, None, unique=unique)
    seconds = time.perf_counter() - t0
    print("caterpillar of %d leaves: %.3f s" % (n, seconds))
    assert root == n and len(parent) == 2 * n - 2
    # the root (t0, rest) dissolves `rest`: children t0, t1, then the chain, numbered down the chain
    assert list(child[n]) == [0, 1, n + 1]
    v = np.arange(n + 1, 2 * n - 2)
    assert np.array_equal(child[v, 0], v - n + 1)
    assert np.array_equal(child[v[:-1], 1], v[:-1] + 1) and child[2 * n - 3, 1] == n - 1
    assert seconds < 1.0
