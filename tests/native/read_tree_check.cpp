// TEST INFRASTRUCTURE: the `-intree` parser (veryfasttree_amd/host/ReadTree.h) as a stand-alone program - no device, no Python.  Built and run
// by tests/test_intree_host_cpu.py, with -fsanitize=address,undefined when asked; needs nothing but a C++11 compiler.
//   read_tree_check [case-file ...]
// First the built-in cases: small trees with known arrays, every malformed text with the message it must be refused with, a polytomy (the
// reference writes past child[3] there), deep nesting and a long caterpillar.  Then every case file (written by the test from a fixture):
//   line 1: n_all n_seqs; then n_all lines "<name> <unique index>"; then n_seqs first rows; the rest of the file is the tree's text.
// For each file one line "case <file's base name> root <r> nodes <n> digest <FNV-1a of parent[] and child[][3] as int64>" or "refused (..)".
// The last line is "failures <k>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../veryfasttree_amd/host/ReadTree.h"

using veryfasttree::ReadTree;
using veryfasttree::ReadTreeResult;

static int failures = 0;

static uint64_t digest(const ReadTreeResult &r) {
    uint64_t h = 1469598103934665603ull;
    auto add = [&](int64_t v) {
        for (int k = 0; k < 8; k++) {
            h ^= (uint64_t) (v >> (8 * k)) & 0xffu;
            h *= 1099511628211ull;
        }
    };
    for (int64_t v: r.parent) add(v);
    for (int64_t v: r.child) add(v);
    return h;
}

struct Aln {
    std::vector<std::string> names;
    std::vector<int64_t> toUniq, first;
};

// names a, b, c, ...; dupOf[k] >= 0: row k repeats row dupOf[k]
static Aln alignment(int n, const std::vector<int> &dupOf = std::vector<int>()) {
    Aln a;
    for (int k = 0; k < n; k++) {
        a.names.push_back(std::string(1, (char) ('a' + k)));
        if (k < (int) dupOf.size() && dupOf[(size_t) k] >= 0) a.toUniq.push_back(a.toUniq[(size_t) dupOf[(size_t) k]]);
        else {
            a.toUniq.push_back((int64_t) a.first.size());
            a.first.push_back(k);
        }
    }
    return a;
}

static std::string show(const ReadTreeResult &r) {
    std::ostringstream o;
    o << "root " << r.root << " parent";
    for (int64_t v: r.parent) o << " " << v;
    o << " child";
    for (int64_t v = (r.nNodes + 2) / 2; v < r.nNodes; v++) o << " [" << r.child[(size_t) (3 * v)] << " " << r.child[(size_t) (3 * v + 1)] << " " << r.child[(size_t) (3 * v + 2)] << "]";
    return o.str();
}

static void expectTree(const char *what, const Aln &a, const std::string &text, const std::string &want, size_t nWarnings = 0) {
    try {
        const ReadTreeResult r = ReadTree::parse(text.data(), text.size(), a.names, a.toUniq, a.first);
        const std::string got = show(r);
        const bool ok = got == want && r.warnings.size() == nWarnings;
        printf("%-28s %s%s\n", what, got.c_str(), ok ? "" : "   <-- WRONG");
        if (!ok) {
            printf("%-28s %s (%zu warnings) expected\n", "", want.c_str(), nWarnings);
            failures++;
        }
    } catch (const std::exception &e) {
        printf("%-28s refused (%s)   <-- WRONG\n", what, e.what());
        failures++;
    }
}

static void expectRefusal(const char *what, const Aln &a, const std::string &text, const std::string &want) {
    try {
        const ReadTreeResult r = ReadTree::parse(text.data(), text.size(), a.names, a.toUniq, a.first);
        printf("%-28s parsed (%s)   <-- WRONG\n", what, show(r).c_str());
        failures++;
    } catch (const std::exception &e) {
        const bool ok = std::string(e.what()).find(want) != std::string::npos;
        printf("%-28s refused (%s)%s\n", what, e.what(), ok ? "" : "   <-- WRONG TEXT");
        if (!ok) failures++;
    }
}

static void builtIn() {
    const Aln a4 = alignment(4), a5 = alignment(5), a6 = alignment(6);
    expectTree("root of two, 4 leaves", a4, "((a,b),(c,d));", "root 4 parent 4 4 5 5 -1 4 child [5 0 1] [2 3 -1]");
    expectTree("root of two, 5 leaves", a5, "((a,b),(c,(d,e)));", "root 5 parent 5 5 6 7 7 -1 5 6 child [6 0 1] [2 7 -1] [3 4 -1]");
    expectTree("lengths, labels, blanks", a5, " ( ( a:0.1 ,b:2e-3)0.95:0.1,\n c ,\t(d:1,e:-0.5)lab:3 ) ;", "root 5 parent 7 7 5 6 6 -1 5 5 child [7 2 6] [3 4 -1] [0 1 -1]", 1);
    expectTree("no semicolon", a4, "(a,b,(c,d))", "root 4 parent 4 4 5 5 -1 4 child [0 1 5] [2 3 -1]");
    // a removed node's children go to the END of its parent's list: (c) leaves [d c], ((a)) leaves [b a]; the root then dissolves its first child
    expectTree("nodes of one child", a4, "((((a)),b),((c),d));", "root 4 parent 4 4 5 5 -1 4 child [5 1 0] [3 2 -1]");
    // rows: a b c d e f with e = copy of a, f = copy of b: the subtree (e,f) holds skipped duplicates only and disappears
    const Aln dup = alignment(6, std::vector<int>{-1, -1, -1, -1, 0, 1});
    expectTree("duplicates-only subtree", dup, "((a,b),((e,f),c),d);", "root 4 parent 5 5 4 4 -1 4 child [5 3 2] [0 1 -1]");   // (.., c) is left with one child: c goes behind d
    expectTree("duplicate named first", dup, "((e,c),(d,(a,b)));", "root 4 parent 4 5 4 5 -1 4 child [5 0 2] [3 1 -1]");
    expectTree("same name twice", a4, "((a,b),(c,(d,a)));", "root 4 parent 4 4 5 5 -1 4 child [5 0 1] [2 3 -1]");
    expectRefusal("leaf only", a4, "a;", "Tree parse error: unexpected token 'a' -- No '(' at start");
    expectRefusal("empty", a4, "  \n", "Tree parse error: unexpected token '(End of file)' -- No '(' at start");
    expectRefusal("'()'", a4, "((),a,b,c,d);", "Tree parse error: unexpected token ')' -- while reading parentheses");
    expectRefusal("';' too early", a4, "((a,b);", "Tree parse error: unexpected token ';' -- unbalanced parentheses");
    expectRefusal("'(' after ')'", a4, "((a,b)(c,d));", "Tree parse error: unexpected token '(' -- unexpected '(' after ')'");
    expectRefusal("bad length", a4, "((a:x,b),(c,d));", "Tree parse error: unexpected token 'x' -- not recognized as a branch length");
    expectRefusal("bad length behind ')'", a4, "((a,b):,(c,d));", "Tree parse error: unexpected token ',' -- not recognized as a branch length");
    expectRefusal("length at the end", a4, "((a,b),(c,d):", "Tree parse error: unexpected token '(End of file)' -- not recognized as a branch length");
    expectRefusal("too many ')'", a4, "(a,b)),(c,d));", "Tree parse error: unexpected token ',' -- too many ')'");
    expectRefusal("stray ';'", a4, "(a,b;c,d);", "Tree parse error: unexpected token ';' -- unexpected token");
    expectRefusal("unknown name", a4, "((a,b),(c,sX));", "Tree parse error: unexpected token 'sX' -- not recognized as a sequence name");
    expectRefusal("a sequence is missing", a5, "((a,b),(c,d));",
                  "Alignment sequence 4 (unique 4) absent from input tree\nThe starting tree (the argument to -intree) must include all sequences in the alignment!");
    expectRefusal("root of four", a4, "(a,b,c,d);", "first leaf is 'a' has more than three children");
    expectRefusal("root of five, nested", a6, "((a,b),c,d,e,f);", "first leaf is 'a' has more than three children");
    expectRefusal("trifurcation below the root", a6, "((a,b,c),d,(e,f));", "first leaf is 'a' has 3 children instead of two");
    expectRefusal("four below the root", a6, "(f,(b,c,d,e),a);", "first leaf is 'b' has more than three children");
    expectRefusal("root of two over three", a5, "((a,b,c),(d,e));", "first leaf is 'a' has 3 children instead of two");   // (d,e) is the child of two that dissolves
    expectRefusal("dissolving overfills", a6, "((a,b),(c,d,e),f);", "first leaf is 'c' has 3 children instead of two");
    // a million '(' in front of the first name, and a caterpillar of 100 000 leaves: nothing recurses, nothing is indexed past its end
    {
        std::string deep(1000000, '(');
        deep += "a" + std::string(1000000, ')') + ",b,(c,d));";
        expectTree("a million nested '('", a4, "(" + deep, "root 4 parent 4 4 5 5 -1 4 child [1 5 0] [2 3 -1]");   // a ends up behind its later siblings
    }
    {
        const int n = 100000;
        Aln big;
        std::string text;
        for (int k = 0; k < n; k++) {
            big.names.push_back("t" + std::to_string(k));
            big.toUniq.push_back(k);
            big.first.push_back(k);
            if (k < n - 1) text += "(t" + std::to_string(k) + ",";
        }
        text += "t" + std::to_string(n - 1) + std::string((size_t) n - 1, ')') + ";";
        try {
            const ReadTreeResult r = ReadTree::parse(text.data(), text.size(), big.names, big.toUniq, big.first);
            // the root dissolves its second child: children t0, t1, then the chain; node ids follow the chain
            bool ok = r.root == n && r.nNodes == 2 * n - 2 && r.child[(size_t) (3 * n)] == 0 && r.child[(size_t) (3 * n + 1)] == 1 && r.child[(size_t) (3 * n + 2)] == n + 1;
            for (int64_t v = n + 1; ok && v < r.nNodes; v++)
                ok = r.parent[(size_t) v] == (v == n + 1 ? n : v - 1) && r.child[(size_t) (3 * v)] == v - n + 1 &&
                     r.child[(size_t) (3 * v + 1)] == (v == r.nNodes - 1 ? n - 1 : v + 1) && r.child[(size_t) (3 * v + 2)] == -1;
            printf("%-28s root %lld nodes %lld%s\n", "caterpillar of 100000", (long long) r.root, (long long) r.nNodes, ok ? "" : "   <-- WRONG");
            if (!ok) failures++;
        } catch (const std::exception &e) {
            printf("%-28s refused (%s)   <-- WRONG\n", "caterpillar of 100000", e.what());
            failures++;
        }
    }
}

static void fromFile(const char *path) {
    std::ifstream in(path, std::ios::binary);
    const char *base = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
    long long nAll = 0, nSeqs = 0;
    if (!(in >> nAll >> nSeqs) || nAll < 1 || nSeqs < 1 || nSeqs > nAll) {
        printf("case %s unreadable\n", base);
        failures++;
        return;
    }
    Aln a;
    for (long long k = 0; k < nAll; k++) {
        std::string nm;
        long long u;
        in >> nm >> u;
        a.names.push_back(nm);
        a.toUniq.push_back(u);
    }
    for (long long u = 0; u < nSeqs; u++) {
        long long k;
        in >> k;
        a.first.push_back(k);
    }
    std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    try {
        const ReadTreeResult r = ReadTree::parse(text.data(), text.size(), a.names, a.toUniq, a.first);
        printf("case %s root %lld nodes %lld digest %016llx\n", base, (long long) r.root, (long long) r.nNodes, (unsigned long long) digest(r));
    } catch (const std::exception &e) {
        printf("case %s refused (%s)\n", base, e.what());
    }
}

int main(int argc, char **argv) {
    builtIn();
    for (int k = 1; k < argc; k++) fromFile(argv[k]);
    printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
