#!/usr/bin/env python3
"""FASTA (nucleotides) -> Newick on one MI355X: the tree `VeryFastTree -nt [-fastest] -noml -nome [-nosupport]` prints,
or - with -mllen - the tree of `VeryFastTree -nt -nome -mllen [-nocat | -cat N] [-nosupport]` (Jukes-Cantor).

    python tools/nj_tree.py in.fasta [-fastest] [-double] [-boot N | -nosupport] [-nj-lengths] [-mllen [-nocat | -cat N]] > tree.nwk
    python tools/nj_tree.py in.fasta -slow [-double] [-nosupport] [-nj-lengths] [-mllen [-nocat | -cat N]] > tree.nwk   # `VeryFastTree -slow ...`
    python tools/nj_tree.py in.fasta -full [-gtr] [-double] [-nosupport] > tree.nwk     # what plain `VeryFastTree -nt [-gtr]` prints
    python tools/nj_tree.py in.fasta -full -lg -double > tree.nwk     # proteins: `VeryFastTree -lg -double-precision` (-aa / -jtt, -wag, -lg)
    python tools/nj_tree.py in.fasta -full -threads 64 [-gamma] [-spr N] > tree.nwk   # the schedule of `VeryFastTree -threads 64`; -gamma; -spr N rounds
    python tools/nj_tree.py in.fasta -intree start.nwk [-mllen ... | -full ...] > tree.nwk   # `VeryFastTree -intree start.nwk ...`: no NJ phase
    python tools/nj_tree.py in.fasta [any mode above] -pseudo [W] > tree.nwk   # `VeryFastTree ... -pseudo [W]`: pseudocount distances
    python tools/nj_tree.py in.fasta -full -spr 4 -mlacc 2 -slownni [-nni N] [-mlnni N] [-sprlength N] > tree.nwk   # the thorough search
    python tools/nj_tree.py in.fasta -aa [-wag | -lg] -full|-mllen -approxml > tree.nwk   # `VeryFastTree ... -approxml` (alias -mlapprox)
    python tools/nj_tree.py -makematrix [-rawdist] [-aa] [-double] in.fasta > matrix.txt   # `VeryFastTree [-nt] [-rawdist] [-double-precision] -makematrix`
    python tools/nj_tree.py in.fasta [any mode above] -rawdist > tree.nwk   # `VeryFastTree ... -rawdist`: no log correction in the ME stages
    python tools/nj_tree.py in.fasta -aa -full|-mllen -trans model.txt > tree.nwk   # `VeryFastTree -trans model.txt ...`: the ML stage under the file's rate matrix
    python tools/nj_tree.py in.fasta [any mode above] -log FILE > tree.nwk   # `VeryFastTree ... -log FILE`: stage trees, likelihoods, rates

Neighbour joining with top hits on the device (veryfasttree_amd/host/NJDriver.h), the root, minimum-evolution branch
lengths (updateBranchLengths), local-bootstrap supports (1000 resamples, reliabilityNJ) and printNJ; -nj-lengths keeps
the NJ branch lengths and prints no supports (the reference's "NJ" log line).  -mllen: maximum-likelihood branch
lengths on that topology (optimizeAllBranchLengths rounds, CAT rate categories unless -nocat) and SH-like supports
(testSplitsML, 1000 resamples) unless -nosupport; the TreeLogLk of every round goes to stderr.
-slow: the exhaustive search of the reference's `-slow` (every join is the best pair of all active nodes, on a distance
matrix kept on the device) instead of top hits; not together with -fastest (as in the reference) or -full (the NNI and
SPR stages of a -slow run are not built).
-intree FILE: the topology of FILE (Newick; branch lengths and labels in it are ignored, duplicate sequences may be named once or
several times, every unique sequence at least once, binary apart from the root) replaces neighbour joining, as the reference's
-intree does; each mode then runs as usual: default = ME lengths and local supports on that topology (`-intree T -noml -nome`),
-mllen = ML lengths and SH-like supports on it (`-intree T -nome -mllen`), -full = refine it (`-intree T`).  Not with -slow.
-makematrix: no tree - the log-corrected distance of every pair of input sequences, computed on the device and printed the
way `VeryFastTree [-nt] [-rawdist] [-double-precision] -makematrix in.fasta` prints it (one row per sequence: its name, then
" %f" per sequence; proteins with -aa: BLOSUM45 distances).  Every sequence is kept (no uniquify); repeated names are an
error; not together with any tree option.
-pseudo [W]: the reference's `-pseudo [weight]`, "recommended if the alignment has sequences with little or no overlap": the
minimum-evolution stages (NNIs, SPR moves, ME branch lengths) estimate the distances of every triplet / quartet with pseudocounts of
weight W (1.0 when no number follows; any W >= 0, 0 = off).  Not read by the NJ phase, the supports, the ML stage and -makematrix.
-mlacc N, -slownni, -nni N, -mlnni N, -sprlength N: the reference's options of the same names, with -full (`-spr 4 -mlacc 2 -slownni` is
the accuracy recipe of FastTree's documentation).  -mlacc N: every quartet of an ML NNI is optimised for N rounds and no alternative is
dropped early, N rounds of the -gtr fit, the supports' second pass always (also with -mllen, for its supports and -gtr).  -slownni: no
subtree is skipped in any NNI round.  -nni N / -mlnni N: N minimum-evolution / ML NNI rounds instead of round(4 log2 n) / round(2 log2 n);
-nni 0 also means -spr 0, -mlnni 0 is -noml.  -sprlength N: SPR chains of at most N steps (default 10, at most 64).  Given without -full
they end the program with a message.
-approxml (or -mlapprox): the reference's option of that name - the posteriors of a protein run's ML stages skip the rotation where one
state dominates and the rest follows the model's near-constant table (NJ.tcc:2390-2421).  Accepted and without effect for nucleotides
and where no ML stage runs, as in the reference.
-rawdist (for a tree): the reference's option of that name - the minimum-evolution NNIs, the SPR chains, the ME branch lengths and the
local-bootstrap supports compare uncorrected profile distances (no Jukes-Cantor / scoredist-like logarithm).  Not read by the NJ phase
and the ML stage, whose starting lengths it changes.
-trans FILE: the reference's option of that name - an amino-acid rate matrix (header `A<tab>R<tab>...<tab>V<tab>*`, then per amino acid its
letter, 20 rates, its stationary frequency) replaces JTT in the ML stage; a -wag / -lg beside it is ignored, as in the reference.  The
file is checked as the reference checks it; proteins only.
-log FILE: the reference's `-log FILE` - the tree after every stage (NJ, ME_NNI<k>, ME_SPR<k>, ME_Lengths, ML_Lengths<k>, ML_NNI<k>), the TreeLogLk
lines, the GTR and rate-category lines, with -gamma the per-site Gamma20 table, the clock lines and the summary; the first line says what the
reference logs and this backend does not (README "-log").  Each line is written when its stage ends.  With -makematrix: that first line alone.
-boot N: N resamples instead of 1000 for the supports, local (default mode) and SH-like (-mllen, -full) alike, as the reference's
-boot; -boot 0 is -nosupport.  Local supports take every alignment the NJ phase takes (10 240 columns).
-full, -mllen, -double, -aa / -jtt and -nj-lengths are this tool's own words; every other flag is the reference's and means what
veryfasttree_amd/refflags.py says it means (a flag it does not know ends the program, as does a flag without its number).
Sequence normalisation and uniquify follow Alignment.cpp:453-526 (U -> T, '.' -> '-', duplicates by sequence string in
first-occurrence order; N -> X for nucleotides)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from veryfasttree_amd import HipProfileOps
from veryfasttree_amd.backend import logging_to, make_matrix, nj_newick, VftError
from veryfasttree_amd.refflags import file_of, from_reference_flags
from veryfasttree_amd.synth import ALPHABET_AA, ALPHABET_NT, NOCODE


def read_fasta(path):
    names, seqs, cur = [], [], []
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if names:
                    seqs.append("".join(cur))
                names.append(line[1:].split()[0] if line[1:].split() else "")
                cur = []
            elif names:
                cur.append(line.strip())
    if names:
        seqs.append("".join(cur))
    return names, seqs


def codes_of(seqs, aa):
    """Alignment.cpp:453-471: '.' -> '-' always; for nucleotides U -> T and N -> X; anything outside the alphabet is NOCODE"""
    seqs = [s.upper().replace(".", "-") for s in seqs]
    if not aa:
        seqs = [s.replace("U", "T").replace("N", "X") for s in seqs]
    lut = np.full(256, NOCODE, np.uint8)
    for i, ch in enumerate(ALPHABET_AA if aa else ALPHABET_NT):
        lut[ord(ch)] = i
    return seqs, np.stack([lut[np.frombuffer(s.encode("ascii", "replace"), np.uint8)] for s in seqs])


NEEDS_FULL = ("-mlacc", "-slownni", "-nni", "-mlnni", "-sprlength")


def translate(args):
    """the tool's command line -> (alignment file, refflags.RefRun of the reference command line it stands for, whether -nj-lengths was
    given): the default mode is the reference's `-noml -nome`, -mllen its `-nome -mllen`, -full its own default; -double is
    -double-precision, -aa / -jtt are the reference without -nt.  Ends the program with a message on anything that cannot run."""
    if not args or args[0].startswith("-"):
        sys.exit(__doc__)
    path, args = args[0], list(args[1:])
    full, mllen = "-full" in args, "-mllen" in args
    if "-slow" in args and full:
        sys.exit("-slow with -full is not built: use -slow alone (the tree of -slow -noml -nome) or with -mllen")
    intree = None
    try:
        args, start = file_of(args, "-intree")
    except ValueError as e:
        sys.exit(str(e))
    if start is not None:
        if "-slow" in args:
            sys.exit("-intree with -slow is not built")
        with open(start) as fh:
            intree = fh.read()
    protein = any(a in args for a in ("-aa", "-jtt", "-wag", "-lg", "-trans"))
    ref = [] if protein else ["-nt"]
    ref += ["-nome", "-mllen"] if mllen else [] if full else ["-noml", "-nome"]
    ref += ["-double-precision" if a == "-double" else a for a in args if a not in ("-full", "-mllen", "-aa", "-jtt", "-nj-lengths")]
    try:
        run = from_reference_flags(ref, intree_text=intree)
    except ValueError as e:
        sys.exit(str(e))
    # an option that cannot take effect is not ignored: all five with -full; -mlacc also with -mllen, whose SH-like supports and -gtr fit
    # read it (NJ.tcc:6934, :6462)
    for flag in NEEDS_FULL:
        if flag in args and not (full or (flag == "-mlacc" and mllen)):
            sys.exit("%s needs -full%s: without it the stage the option belongs to does not run" % (flag, " or -mllen" if flag == "-mlacc" else ""))
    unbuilt = [key for key in run.other if key not in ("log", "rawdist", "trans")]
    if unbuilt:
        sys.exit("not built in this tool: -%s" % ", -".join(unbuilt))
    if "trans" in run.other:   # (refflags opens no file: the text goes on as nj_newick's aa_trans)
        try:
            with open(run.other["trans"], "rb") as fh:
                run.kwargs["aa_trans"] = fh.read()
        except OSError as e:
            sys.exit("-trans %s: %s" % (run.other["trans"], e.strerror))
    if "rawdist" in run.other:
        run.kwargs["rawdist"] = True
    nj_len = "-nj-lengths" in args
    return path, run._replace(n_bootstrap=0 if nj_len else run.n_bootstrap), nj_len


MAKEMATRIX_FLAGS = ("-makematrix", "-rawdist", "-aa", "-double")


def main_makematrix(args):
    """`-makematrix`: every sequence of the alignment, in input order, against every sequence"""
    try:
        args, log = file_of(args, "-log")   # (the log of a -makematrix run is its first line)
    except ValueError as e:
        sys.exit(str(e))
    other = [a for a in args if a.startswith("-") and a not in MAKEMATRIX_FLAGS]
    if other:
        sys.exit("-makematrix prints distances and builds no tree: it cannot be combined with %s (allowed: -rawdist, -aa, -double)" % " ".join(other))
    paths = [a for a in args if not a.startswith("-")]
    if len(paths) != 1:
        sys.exit("-makematrix needs exactly one alignment file")
    names, seqs = read_fasta(paths[0])
    if not seqs or len({len(s) for s in seqs}) != 1:
        sys.exit("sequences have different lengths: not an alignment")
    aa = "-aa" in args
    _, codes_all = codes_of(seqs, aa)
    sys.stdout.flush()
    try:   # the text goes to standard output, as the reference's does even with -out
        with logging_to(log):
            make_matrix(codes_all, names, 20 if aa else 4, np.float64 if "-double" in args else np.float32, "-rawdist" in args, 1)
    except VftError as e:
        sys.exit(str(e))


def main():
    args = sys.argv[1:]
    if "-makematrix" in args:
        return main_makematrix(args)
    path, run, nj_len = translate(args)
    names, seqs = read_fasta(path)
    if len({len(s) for s in seqs}) != 1:
        sys.exit("sequences have different lengths: not an alignment")
    seqs, codes_all = codes_of(seqs, run.n_codes == 20)   # (the sequences are uniquified as strings, after the normalisation)
    first_of, last, unique_first = {}, {}, []
    aln_next = np.full(len(seqs), -1, np.int64)
    for k, s in enumerate(seqs):
        if s not in first_of:
            first_of[s] = k
            unique_first.append(k)
        else:
            aln_next[last[s]] = k
        last[s] = k
    if len(unique_first) < 3:
        sys.exit("fewer than 3 unique sequences")
    try:
        tree, loglk = nj_newick(lambda n, L: HipProfileOps(n, L, run.n_codes, run.dtype, max_nodes=3 * n), codes_all, names, me_lengths=not nj_len,
                                unique=(np.array(unique_first, np.int64), aln_next), n_bootstrap=run.n_bootstrap, return_loglk=True, log=run.other.get("log"), **run.kwargs)
    except OSError as e:
        if run.other.get("log") is None or e.filename != run.other["log"]:   # (only the log's own file is opened on the way)
            raise
        sys.exit("-log %s: %s" % (e.filename, e.strerror))
    except VftError as e:
        if "intree" not in run.kwargs and "aa_trans" not in run.kwargs and "-log" not in str(e):
            raise
        sys.exit(str(e))
    label = "Round" if "ml_nni" in run.kwargs else "Length"   # of the TreeLogLk lines: by the stages that run, whatever -mlacc adds to a -mllen run
    for k, ll in enumerate(loglk):
        sys.stderr.write("TreeLogLk\t%s%d\t%.4f\n" % (label, k + 1, ll))
    print(tree)


if __name__ == "__main__":
    main()
