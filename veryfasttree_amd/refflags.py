"""The one translation from the reference's command line to this backend's options (no device, no ctypes).

from_reference_flags(["-nt", "-spr", "4", "-mlacc", "2", "-slownni"]) -> RefRun: the alphabet, the precision, the number of resamples
and the keyword arguments of backend.nj_newick that run what `VeryFastTree <flags>` runs.  The fixtures under tests/golden/ store such
flags (`flags` / `rN_flags`); the tests, tools/nj_tree.py and the measuring tools all come through here, so a flag means one thing.
The stages follow the reference's own option handling (main.cpp:189-212, :270-275, :306-316; VeryFastTree.cpp:72, :87-91, :109-111)."""
import collections
import math

import numpy as np

RefRun = collections.namedtuple("RefRun", "n_codes dtype n_bootstrap kwargs other")
RefRun.__doc__ = """n_codes: 4 with -nt, else 20; dtype: np.float64 with -double-precision, else np.float32 (also kwargs["dtype"]);
n_bootstrap: `-boot N`, 0 with -nosupport, else 1000; kwargs: the keyword arguments of nj_newick, only those the flags ask for;
other: what the caller has to act on - makematrix, notop (True), seed (int), log (the file name of `-log FILE`: this module opens no
file - the caller hands it to nj_newick(log=...)), rawdist (True: with makematrix the matrix's own switch, else nj_newick(rawdist=True)),
trans (the file name of `-trans FILE`: the caller reads it and hands the text to nj_newick(aa_trans=...), which then ignores aa_model,
as the reference ignores -wag / -lg beside -trans)."""

SWITCHES = ("-nt", "-double-precision", "-lg", "-wag", "-gtr", "-gamma", "-noml", "-nome", "-mllen", "-nocat", "-nosupport", "-slow",
            "-fastest", "-2nd", "-no2nd", "-notop", "-slownni", "-makematrix", "-rawdist", "-approxml", "-mlapprox")
# flag: (least, most, what the message asks for beyond "a whole number")
COUNTS = {"-spr": (0, None, ">= 0"), "-mlacc": (1, None, ">= 1"), "-nni": (0, None, ">= 0"), "-mlnni": (0, None, ">= 0"),
          "-sprlength": (1, 64, "from 1 to 64 (the SPR chain buffers hold 64 steps)"), "-cat": (1, None, ">= 1"),
          "-boot": (0, None, "of resamples >= 0"), "-threads": (1, None, ">= 1"), "-seed": (None, None, "")}
THOROUGH = {"-mlacc": "ml_accuracy", "-nni": "nni_rounds", "-mlnni": "ml_nni_rounds", "-sprlength": "spr_length"}


def zero_round_stages(me_nni, spr, ml_nni, nni_rounds, ml_nni_rounds):
    """`-nni 0` is no minimum-evolution NNI round and no SPR round either (VeryFastTree.cpp:72); `-mlnni 0` is no ML NNI round.
    Returns (me_nni, spr, ml_nni) with a count of 0 applied; None or a positive count leaves them alone."""
    if nni_rounds is not None and int(nni_rounds) == 0:
        me_nni, spr = False, 0
    if ml_nni_rounds is not None and int(ml_nni_rounds) == 0:
        ml_nni = 0
    return me_nni, spr, ml_nni


def file_of(flags, flag):
    """(the flags without `flag FILE`, FILE or None) for a flag that takes a file name (-log, -intree, -trans); a ValueError that names the flag
    where the name is missing or the flag is given twice.  Callers that keep flags of their own next to the reference's (tools/nj_tree.py)
    take the file out with this before they look at the rest."""
    flags = list(flags)
    if flags.count(flag) > 1:
        raise ValueError("%s is given twice" % flag)
    if flag not in flags:
        return flags, None
    k = flags.index(flag)
    if k + 1 >= len(flags):
        raise ValueError("%s needs a file" % flag)
    return flags[:k] + flags[k + 2:], flags[k + 1]


def _parse(flags):
    """{flag: True or its number}; -pseudo takes the next token as its weight if that is a number, else 1.0 (main.cpp:165-175)"""
    seen, k = {}, 0
    while k < len(flags):
        flag = flags[k]
        k += 1
        if flag in seen:
            raise ValueError("%s is given twice" % flag)
        if flag in SWITCHES:
            seen[flag] = True
        elif flag in COUNTS:
            least, most, wanted = COUNTS[flag]
            try:
                value = int(flags[k])
            except (IndexError, ValueError):
                raise ValueError("%s needs a whole number" % flag) from None
            if (least is not None and value < least) or (most is not None and value > most):
                raise ValueError("%s needs a number %s, not %d" % (flag, wanted, value))
            seen[flag] = value
            k += 1
        elif flag == "-pseudo":
            weight = 1.0
            if k < len(flags):
                try:
                    weight = float(flags[k])
                    k += 1
                except ValueError:
                    pass
            if not (weight >= 0.0) or math.isinf(weight):
                raise ValueError("-pseudo takes a weight >= 0, not '%s'" % flags[k - 1])
            seen[flag] = weight
        else:
            raise ValueError("%s: not a flag of the reference that this backend knows" % flag)
    return seen


def from_reference_flags(flags, threads=None, intree_text=None):
    """flags: the reference's arguments, a list or a space-joined string.  threads: the run's `-threads T` where the flags do not carry
    it (the fixtures store it apart).  intree_text: the Newick text of `-intree FILE` - this function opens no file, so flags that name
    one need the text; the text alone is taken as `-intree`.  An unknown flag, a flag without its number and a number out of range are
    a ValueError that names the flag."""
    flags, files = flags.split() if isinstance(flags, str) else list(flags), {}
    for flag in ("-intree", "-log", "-trans"):
        flags, name = file_of(flags, flag)
        if name is not None:
            files[flag] = name
    f = dict(_parse(flags), **files)
    nt = "-nt" in f
    dtype = np.float64 if "-double-precision" in f else np.float32
    kw = dict(dtype=dtype)
    models = [m for m in ("-lg", "-wag") if m in f]
    if models and (nt or len(models) > 1):
        raise ValueError("%s is one amino-acid model: not with %s" % (models[-1], "-nt" if nt else models[0]))
    if "-trans" in f and nt:
        raise ValueError("-trans %s is an amino-acid model: not with -nt" % f["-trans"])   # (VeryFastTree.cpp:100)
    if not nt:
        kw["aa_model"] = models[0][1:] if models else "jtt"
    if "-slow" in f and "-fastest" in f:
        raise ValueError("-slow and -fastest exclude each other")
    if "-threads" in f and threads is not None and int(threads) != f["-threads"]:
        raise ValueError("-threads %d in the flags, threads=%d beside them" % (f["-threads"], int(threads)))
    threads = f.get("-threads", threads)
    if threads is not None:
        kw["threads"] = int(threads)
    if "-fastest" in f:
        kw["fastest"] = True
    if "-2nd" in f and "-no2nd" in f:
        raise ValueError("-2nd and -no2nd exclude each other")
    if "-2nd" in f or "-no2nd" in f or ("-fastest" in f and kw.get("threads", 1) > 1):   # (VeryFastTree.cpp:87-91: never at T > 1)
        kw["second_level"] = "-2nd" in f and kw.get("threads", 1) <= 1
    if "-slow" in f:
        kw["slow"] = True
    if "-pseudo" in f:
        kw["pseudo"] = f["-pseudo"]
    if "-intree" in f and intree_text is None:
        raise ValueError("-intree %s: pass the file's text as intree_text" % f["-intree"])
    if intree_text is not None:
        kw["intree"] = intree_text
    # the stages (main.cpp: -nome is -nni 0 -spr 0; -noml is -mlnni 0; -mllen is that plus the length rounds)
    if "-nocat" in f and "-cat" in f:
        raise ValueError("-nocat and -cat exclude each other")
    cats = 1 if "-nocat" in f else f.get("-cat", 20)
    me_nni = "-nome" not in f
    ml_nni = 0 if ("-noml" in f or "-mllen" in f) else cats
    me_nni, spr, ml_nni = zero_round_stages(me_nni, f.get("-spr", 2) if me_nni else 0, ml_nni, f.get("-nni"), f.get("-mlnni"))
    if me_nni:
        kw.update(me_nni=True, spr=spr)
    if "-mllen" in f:
        kw["mllen"] = cats
    elif ml_nni:
        kw["ml_nni"] = ml_nni
    if "-mllen" in f or ml_nni:
        kw.update({key: True for key in ("gtr", "gamma") if "-" + key in f})
    if "-slownni" in f:
        kw["slow_nni"] = True
    # -approxml / -mlapprox (main.cpp:216, one option with two names): posteriorProfile reads it for 20 states alone, and only an ML
    # stage computes posteriors - under -nt or -noml the reference accepts it and nothing changes, so it translates to nothing
    if "-approxml" in f and "-mlapprox" in f:
        raise ValueError("-mlapprox is -approxml under its other name: the option is given twice")
    if ("-approxml" in f or "-mlapprox" in f) and not nt and ("-mllen" in f or ml_nni):
        kw["approx_ml"] = True
    kw.update({key: f[flag] for flag, key in THOROUGH.items() if f.get(flag)})   # (a count of 0 has become the switches above)
    n_bootstrap = 0 if "-nosupport" in f else f.get("-boot", 1000)
    other = {key: f["-" + key] for key in ("makematrix", "rawdist", "notop", "seed", "log", "trans") if "-" + key in f}
    return RefRun(4 if nt else 20, dtype, n_bootstrap, kw, other)
