"""The lines of a `-log FILE` that this backend writes and the reference writes too (no device, no ctypes): which lines of the
reference's log are in scope, how their clock fields are masked, and what to call a line in a message.  The fixture generator
(tools/gen_log_fixtures.py), the tests and the tools compare logs through here, so "the same log" means one thing.

In scope: the stage trees, `Min_evolution NNIs converged`, the TreeLogLk lines, what setMLGtr / setMLRates /
logMLRates print, the Gamma lines and table, the clock lines, `NNI: .. SPR: .. ML-NNI: ..` and `TreeCompleted`.  Everything else the
reference logs - command, version and option echo, operation counts, progress and warning texts - is out of scope, as is this
backend's own first line."""
import re

HEADER_PREFIX = "# veryfasttree-amd log:"

TREE_TAG = r"(?:NJ|ME_NNI\d+|ME_SPR\d+|ME_Lengths|ML_Lengths\d*|ML_NNI\d+)"
IN_SCOPE = re.compile("|".join([
    r"^%s\t" % TREE_TAG,
    r"^Min_evolution NNIs converged at round \d+ -- skipping some rounds$",
    r"^TreeLogLk\t",
    r"^GTR Frequencies: ", r"^GTR rates\(ac ag at cg ct gt\) ",
    r"^Switched to using \d+ rate categories \(CAT approximation\)$", r"^Rate categories were divided by ", r"^CAT-based log-likelihoods may not be comparable across runs$",
    r"^NCategories\d+$", r"^Rates ", r"^SiteCategories ",
    r"^Gamma\d+LogLk\t", r"^Gamma\d+\t",
    r"^Initial topology in ", r"^Refining topology: ", r"^Total branch-length ", r"^\d+ rounds ML lengths: ", r"^ML-NNI round \d+: ",
    r"^Turning off heuristics for final round of ML NNIs", r"^Optimize all lengths: ", r"^Gamma\(\d+\) LogLk ", r"^Total time: ",
    r"^NNI: \d+ SPR: \d+ ML-NNI: \d+$",
    r"^TreeCompleted$"]))

# the clock fields: the only numbers of an in-scope line that differ between two runs of the same program
CLOCKS = [(re.compile(r"^(Initial topology in )\d+\.\d\d( seconds)$"), r"\1#\2"),
          (re.compile(r"^(Total branch-length -?\d+\.\d{3} after )\d+\.\d\d( sec)$"), r"\1#\2"),
          (re.compile(r"^(\d+ rounds ML lengths: .* Time )\d+\.\d\d$"), r"\1#"),
          (re.compile(r"^(ML-NNI round \d+: .* Time )\d+\.\d\d((?: \(final\))?)$"), r"\1#\2"),
          (re.compile(r"^(Optimize all lengths: .* Time )\d+\.\d\d$"), r"\1#"),
          (re.compile(r"^(Total time: )\d+\.\d\d( seconds )"), r"\1#\2")]


def in_scope(line):
    return bool(IN_SCOPE.match(line))


def mask(line):
    """the line with its clock field replaced by `#`; any other line as it is"""
    for pattern, to in CLOCKS:
        line, n = pattern.subn(to, line)
        if n:
            break
    return line


def tag(line):
    """what a message calls the line: `ME_SPR1`, `TreeLogLk ML_NNI2`, `Gamma20 17` (a table row), else its first two words"""
    fields = line.split("\t")
    if re.fullmatch(TREE_TAG, fields[0]):
        return fields[0]
    if len(fields) > 1:
        return " ".join(fields[:2])
    return " ".join(line.split(" ")[:2])


def masked_lines(text):
    """the in-scope lines of a log's text, in order, clocks masked"""
    return [mask(line) for line in text.split("\n") if in_scope(line)]


def first_difference(got, want):
    """None where the two lists of masked lines are the same, else a message that names the first differing line's tag"""
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return "line %d, %s: got %r, the reference has %r" % (k, tag(b), a[:200], b[:200])
    if len(got) != len(want):
        longer = got if len(got) > len(want) else want
        return "%d lines, the reference has %d: the first one without a partner is %s" % (len(got), len(want), tag(longer[min(len(got), len(want))]))
    return None
