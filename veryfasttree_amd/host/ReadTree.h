// `-intree`: a starting tree in Newick text -> the node arrays NJDriver::readTree installs.  Pure host code, no device, no recursion.
//
// Restates NeighbourJoining::readTree up to its node numbering (NJ.tcc:2449-2665 with readTreeToken :3316-3340, readTreeMaybeAddLeaf
// :3250-3274, readTreeRemove :3276-3314):
//   tokens    ( ) : ; , stand alone, white space ends a token, everything else accumulates - no quoting;
//   parse     a stack of open nodes; branch lengths and numeric labels are dropped, any other label after ')' is a warning;
//   leaves    a name is looked up among the names of the WHOLE alignment and mapped to its unique sequence; the first occurrence of a
//             unique sequence becomes a leaf, later ones (other names of the same sequence, the same name again) are skipped;
//   complete  every unique sequence must have been seen;
//   simplify  until nothing changes: non-root internal nodes with fewer than two children are removed (their children go to the END of
//             the parent's list), a root with one child hands the root over; then a root of two dissolves its first child of two;
//   numbering leaves keep their unique index, internal nodes get nSeqs, nSeqs + 1, ... in the order a stack pops them (root first,
//             children pushed in list order, the last pushed popped first) - the root is nSeqs, NOT the highest id as after fastNJ.
// Where the reference only has asserts (compiled out of its release build; a polytomy writes past child[3] there) this code refuses: no
// node ever holds more than three children, and after the simplification every non-root internal node has exactly two and the root
// exactly three.
#ifndef VFT_READ_TREE_H
#define VFT_READ_TREE_H

#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace veryfasttree {

    struct ReadTreeResult {
        std::vector<int64_t> parent;   /* [nNodes], -1 at the root */
        std::vector<int64_t> child;    /* [nNodes][3], -1 = none; leaves have none, the root three */
        int64_t root = -1, nNodes = 0;
        std::vector<std::string> warnings;
    };

    class ReadTree {
    public:
        /* names[k] = name of alignment row k; alnToUniq[k] = its unique sequence; uniqueFirst[u] = first row of unique sequence u
           (error texts only) */
        static ReadTreeResult parse(const char *text, size_t len, const std::vector<std::string> &names, const std::vector<int64_t> &alnToUniq,
                                    const std::vector<int64_t> &uniqueFirst) {
            ReadTree t(text, len, names, alnToUniq, uniqueFirst);
            t.readTokens();
            t.checkComplete();
            t.simplify();
            return t.number();
        }

    private:
        struct Children {
            int64_t child[3];
            int nChild;
        };

        const char *text;
        size_t len, pos = 0;
        const std::vector<std::string> &names;
        const std::vector<int64_t> &alnToUniq, &uniqueFirst;
        const int64_t nSeqs;
        std::unordered_map<std::string, int64_t> byName;
        std::vector<int64_t> parent;       /* parse ids: leaves 0 .. nSeqs-1, internal nodes from nSeqs on in the order they open */
        std::vector<Children> children;
        int64_t root;
        ReadTreeResult res;

        ReadTree(const char *text, size_t len, const std::vector<std::string> &names, const std::vector<int64_t> &alnToUniq,
                 const std::vector<int64_t> &uniqueFirst)
                : text(text), len(len), names(names), alnToUniq(alnToUniq), uniqueFirst(uniqueFirst), nSeqs((int64_t) uniqueFirst.size()) {
            if (names.size() != alnToUniq.size()) throw std::invalid_argument("readTree: one unique index per alignment name is needed");
            byName.reserve(names.size() * 2);
            for (size_t k = 0; k < names.size(); k++) {
                if (alnToUniq[k] < 0 || alnToUniq[k] >= nSeqs) throw std::invalid_argument("readTree: unique index out of range");
                if (!byName.emplace(names[k], (int64_t) k).second)
                    throw std::invalid_argument("Non-unique name '" + names[k] + "' in the alignment");
            }
            parent.assign((size_t) nSeqs, -1);
            children.assign((size_t) nSeqs, Children{{-1, -1, -1}, 0});
            root = newNode();
        }

        int64_t newNode() {
            parent.push_back(-1);
            children.push_back(Children{{-1, -1, -1}, 0});
            return (int64_t) parent.size() - 1;
        }

        static bool isSpace(int c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

        static bool startsNumber(const std::string &tok) { return !tok.empty() && (tok[0] == '-' || (tok[0] >= '0' && tok[0] <= '9')); }

        bool token(std::string &buf) {
            buf.clear();
            while (pos < len) {
                const char c = text[pos];
                if (c == '(' || c == ')' || c == ':' || c == ';' || c == ',') {
                    if (buf.empty()) {
                        buf += c;
                        pos++;
                    }
                    break;
                }
                pos++;
                if (isSpace((unsigned char) c)) {
                    if (!buf.empty()) break;
                } else buf += c;
            }
            return !buf.empty();
        }

        [[noreturn]] static void parseError(const char *what, const std::string &tok) {
            throw std::invalid_argument("Tree parse error: unexpected token '" + (tok.empty() ? std::string("(End of file)") : tok) + "' -- " + what);
        }

        /* the name of the first leaf below a node, children in list order (error texts) */
        std::string firstLeafName(int64_t node) const {
            std::vector<int64_t> stack(1, node);
            while (!stack.empty()) {
                const int64_t v = stack.back();
                stack.pop_back();
                if (v < nSeqs) return names[(size_t) uniqueFirst[(size_t) v]];
                for (int k = children[(size_t) v].nChild - 1; k >= 0; k--) stack.push_back(children[(size_t) v].child[k]);
            }
            return "(no leaf)";
        }

        [[noreturn]] void refuse(int64_t node, const std::string &what) const {
            throw std::invalid_argument("The starting tree must be binary: the node whose first leaf is '" + firstLeafName(node) + "' " + what);
        }

        void addChild(int64_t p, int64_t c) {
            Children &pc = children[(size_t) p];
            if (pc.nChild == 3) refuse(p, "has more than three children");
            parent[(size_t) c] = p;
            pc.child[pc.nChild++] = c;
        }

        void maybeAddLeaf(int64_t p, const std::string &name) {
            const auto it = byName.find(name);
            if (it == byName.end()) parseError("not recognized as a sequence name", name);
            const int64_t u = alnToUniq[(size_t) it->second];
            if (parent[(size_t) u] < 0) addChild(p, u);   /* else: seen already, skipped */
        }

        void readBranchLength(std::string &tok) {
            if (!token(tok) || !startsNumber(tok)) parseError("not recognized as a branch length", tok);
        }

        void readTokens() {
            std::vector<int64_t> stack(1, root);   /* the path from the root to the open node */
            int64_t nDown = 0, nUp = 0;
            std::string tok;
            if (!token(tok) || tok[0] != '(') parseError("No '(' at start", tok);
            while (token(tok)) {
                const char c = tok[0];
                if (nDown > 0) {   /* in a run of '(' */
                    if (c == '(') nDown++;
                    else if (c == ',' || c == ';' || c == ':' || c == ')') parseError("while reading parentheses", tok);
                    else {
                        for (; nDown > 0; nDown--) {
                            const int64_t node = newNode();
                            addChild(stack.back(), node);
                            stack.push_back(node);
                        }
                        maybeAddLeaf(stack.back(), tok);
                    }
                } else if (nUp > 0) {   /* behind a run of ')' */
                    if (c == ';') {
                        if (nUp != (int64_t) stack.size()) parseError("unbalanced parentheses", tok);
                        break;
                    } else if (c == ')') nUp++;
                    else if (c == '(') parseError("unexpected '(' after ')'", tok);
                    else if (c == ':') readBranchLength(tok);
                    else if (c == ',') {
                        for (; nUp > 0; nUp--) {
                            stack.pop_back();
                            if (stack.empty()) parseError("too many ')'", tok);
                        }
                    } else if (!startsNumber(tok))
                        res.warnings.push_back("Warning while parsing tree: non-numeric label " + tok + " for internal node");
                } else if (c == '(') nDown = 1;
                else if (c == ')') nUp = 1;
                else if (c == ':') readBranchLength(tok);
                else if (c == ',') {
                } else if (c == ';') parseError("unexpected token", tok);
                else maybeAddLeaf(stack.back(), tok);
            }
        }

        void checkComplete() const {
            for (int64_t u = 0; u < nSeqs; u++)
                if (parent[(size_t) u] < 0)
                    throw std::invalid_argument("Alignment sequence " + std::to_string(uniqueFirst[(size_t) u]) + " (unique " + std::to_string(u) +
                                                ") absent from input tree\n"
                                                "The starting tree (the argument to -intree) must include all sequences in the alignment!");
        }

        /* readTreeRemove: the node leaves its parent's list, the later siblings move down, its children go to the end */
        void removeNode(int64_t node) {
            const int64_t p = parent[(size_t) node];
            parent[(size_t) node] = -1;
            Children &pc = children[(size_t) p];
            int at = 0;
            while (at < pc.nChild && pc.child[at] != node) at++;
            for (int k = at; k < pc.nChild - 1; k++) pc.child[k] = pc.child[k + 1];
            pc.nChild--;
            Children &nc = children[(size_t) node];
            if (pc.nChild + nc.nChild > 3) {
                parent[(size_t) node] = p;   /* (the text names a leaf below the parent) */
                refuse(p, "would hold more than three children once a node above it is dissolved");
            }
            for (int k = 0; k < nc.nChild; k++) {
                pc.child[pc.nChild++] = nc.child[k];
                parent[(size_t) nc.child[k]] = p;
            }
            for (int k = pc.nChild; k < 3; k++) pc.child[k] = -1;
            nc.nChild = 0;
            nc.child[0] = nc.child[1] = nc.child[2] = -1;
        }

        void simplify() {
            std::vector<int64_t> stack;
            int64_t nRemoved;
            do {
                nRemoved = 0;
                stack.assign(1, root);
                while (!stack.empty()) {
                    const int64_t node = stack.back();
                    stack.pop_back();
                    if (node < nSeqs) continue;
                    Children &c = children[(size_t) node];
                    if (c.nChild <= 1) {
                        if (node != root) {
                            removeNode(node);
                            nRemoved++;
                        } else if (c.nChild == 1) {
                            const int64_t newroot = c.child[0];
                            parent[(size_t) newroot] = -1;
                            c.nChild = 0;
                            nRemoved++;
                            root = newroot;
                            stack.push_back(newroot);
                        }
                    } else
                        for (int k = 0; k < c.nChild; k++) stack.push_back(c.child[k]);
                }
            } while (nRemoved > 0);
            if (root < nSeqs) throw std::invalid_argument("The starting tree must be binary: it holds a single leaf");
            if (children[(size_t) root].nChild == 2)   /* root -> child -> A, B becomes root -> A, B */
                for (int k = 0; k < 2; k++) {
                    const int64_t ch = children[(size_t) root].child[k];
                    if (children[(size_t) ch].nChild == 2) {
                        removeNode(ch);
                        break;
                    }
                }
        }

        ReadTreeResult number() {
            /* the binary check first: the arrays below have room for a binary tree only */
            std::vector<int64_t> stack(1, root), order;
            while (!stack.empty()) {
                const int64_t node = stack.back();
                stack.pop_back();
                if (node < nSeqs) continue;
                const Children &c = children[(size_t) node];
                if (node == root && c.nChild != 3) refuse(node, "is the root and has " + std::to_string(c.nChild) + " children instead of three");
                if (node != root && c.nChild != 2) refuse(node, "has " + std::to_string(c.nChild) + " children instead of two");
                order.push_back(node);
                for (int k = 0; k < c.nChild; k++) stack.push_back(c.child[k]);
            }
            std::vector<int64_t> map(parent.size(), -1);
            for (int64_t u = 0; u < nSeqs; u++) map[(size_t) u] = u;
            int64_t maxnode = nSeqs;
            for (int64_t node: order) map[(size_t) node] = maxnode++;
            if (maxnode != 2 * nSeqs - 2) throw std::invalid_argument("readTree: the simplified tree does not hold every sequence once");
            res.nNodes = maxnode;
            res.root = map[(size_t) root];
            res.parent.assign((size_t) maxnode, -1);
            res.child.assign((size_t) (3 * maxnode), -1);
            for (size_t node = 0; node < parent.size(); node++) {
                const int64_t nj = map[node];
                if (nj < 0) continue;
                for (int k = 0; k < children[node].nChild; k++) res.child[(size_t) (3 * nj + k)] = map[(size_t) children[node].child[k]];
                if (parent[node] >= 0) res.parent[(size_t) nj] = map[(size_t) parent[node]];
            }
            return res;
        }
    };

}

#endif
