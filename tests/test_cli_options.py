"""ribbit-hip's argument handling for the row outputs (--masked-fasta, --repeat-fasta, --loci-bed, --density-bedgraph and their
qualifiers): every command line here ends in an error message or the help text before the tool touches a GPU, so none of this
needs one.  Exit status 1 and the exact text on stderr."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
pytestmark = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")

# file option, then its qualifiers with a value each takes; in the order the tool checks and opens them
OUTPUTS = [("--masked-fasta", [("--mask", "hard"), ("--mask-width", "7")]),
           ("--repeat-fasta", [("--flank", "5")]),
           ("--loci-bed", [("--loci-gap", "3")]),
           ("--density-bedgraph", [("--density-window", "500")])]
QUALIFIERS = [(q, v, owner) for owner, quals in OUTPUTS for q, v in quals]
BASES = "wants a whole number of bases"


def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == message, args
    return r


def _dies(args, message):
    return _fails(args, "ribbit-hip: " + message + "\n")


@pytest.mark.parametrize("qualifier,value,owner", QUALIFIERS)
def test_qualifier_without_its_owner(qualifier, value, owner):
    _dies([qualifier, value], f"{qualifier} needs {owner}")
    _dies(["-i", "in.fa", f"{qualifier}={value}"], f"{qualifier} needs {owner}")
    # somebody else's owner does not help
    other = next(o for o, _ in OUTPUTS if o != owner)
    _dies([qualifier, value, other, "out"], f"{qualifier} needs {owner}")


def test_both_mask_qualifiers_without_masked_fasta_name_mask():
    _dies(["--mask", "soft", "--mask-width", "9"], "--mask needs --masked-fasta")
    _dies(["--mask-width", "9", "--mask", "hard"], "--mask needs --masked-fasta")


def test_of_two_orphans_the_first_in_the_order_of_the_outputs_is_reported():
    firsts = [(quals[-1][0], quals[-1][1], owner) for owner, quals in OUTPUTS]      # --mask-width, --flank, --loci-gap, --density-window
    for a in range(len(firsts)):
        for b in range(a + 1, len(firsts)):
            (qa, va, oa), (qb, vb, _) = firsts[a], firsts[b]
            _dies([qb, vb, qa, va], f"{qa} needs {oa}")
            _dies([qa, va, qb, vb], f"{qa} needs {oa}")
    _dies(["--density-window", "5", "--loci-gap", "1", "--flank", "2", "--mask", "hard"], "--mask needs --masked-fasta")


@pytest.mark.parametrize("option", [o for o, _ in OUTPUTS])
def test_empty_file_name(option):
    _dies([option + "="], f"{option} wants a file name")
    _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")


@pytest.mark.parametrize("option,value,wants", [
    ("--mask", "medium", "wants soft or hard"),
    ("--mask-width", "-1", BASES + " (0 or more)"),
    ("--mask-width", "x", BASES + " (0 or more)"),
    ("--mask-width", "1234567890", BASES + " (0 or more)"),
    ("--flank", "-1", BASES + " (0 or more, at most 9 digits)"),
    ("--flank", "1234567890", BASES + " (0 or more, at most 9 digits)"),
    ("--loci-gap", "2147483648", BASES + " (0 .. 2147483647)"),
    ("--loci-gap", "x", BASES + " (0 .. 2147483647)"),
    ("--density-window", "0", BASES + " (1 .. 2147483647)"),
    ("--density-window", "2147483648", BASES + " (1 .. 2147483647)"),
])
def test_rejected_qualifier_values(option, value, wants):
    owner = next(o for q, _, o in QUALIFIERS if q == option)
    _dies([option, value], f"{option} {wants}, got '{value}'")
    _dies(["-i", "in.fa", owner, "out", f"{option}={value}"], f"{option} {wants}, got '{value}'")


def _cannot_open(option, path):
    return f"{option}: cannot open '{path}' for writing"


@pytest.mark.parametrize("owner,qualifier,value", [("--loci-bed", "--loci-gap", "2147483647"), ("--density-bedgraph", "--density-window", "1"),
                                                   ("--loci-bed", "--loci-gap", "0"), ("--density-bedgraph", "--density-window", "2147483647"),
                                                   ("--masked-fasta", "--mask-width", "999999999"), ("--masked-fasta", "--mask-width", "0"),
                                                   ("--repeat-fasta", "--flank", "999999999"), ("--repeat-fasta", "--flank", "0")])
def test_accepted_limits_parse_and_reach_the_files(tmp_path, owner, qualifier, value):
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", qualifier, value, owner, out], _cannot_open(owner, out))


@pytest.mark.parametrize("option", [o for o, _ in OUTPUTS])
def test_unwritable_output_path(tmp_path, option):
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", option, out], _cannot_open(option, out))
    _dies(["-i", tmp_path / "in.fa", f"{option}={out}"], _cannot_open(option, out))
    assert not (tmp_path / "missing").exists()


def test_files_are_opened_in_the_order_of_the_outputs(tmp_path):
    """whatever the order on the command line: masked, repeat, loci, density.  An output before the one that cannot be opened exists
    afterwards, one behind it does not."""
    options = [o for o, _ in OUTPUTS]
    for bad in range(len(options)):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa"]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, _cannot_open(options[bad], paths[bad]))
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]
        assert all(p.read_bytes() == b"" for p in paths[:bad])
    # two that cannot be opened: the first in that order is the one reported
    for a in range(len(options)):
        for b in range(a + 1, len(options)):
            out = tmp_path / "missing" / "out"
            _dies(["-i", tmp_path / "in.fa", options[b], out, options[a], out], _cannot_open(options[a], out))


def test_other_option_errors(tmp_path):
    _dies(["--bogus"], "unrecognised option '--bogus'")
    _dies(["-i", "in.fa", "--loci=x"], "unrecognised option '--loci=x'")
    _dies(["-x"], "unrecognised option '-x'")
    _dies(["-W", "5"], "unrecognised option '-W'")
    for option in [o for o, _ in OUTPUTS] + [q for q, _, _ in QUALIFIERS] + ["-i", "--timing"]:
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    _dies(["in.fa"], "too many positional options have been specified on the command line")
    _dies(["-i", "in.fa", "--flank", "5", "stray"], "too many positional options have been specified on the command line")
    _dies(["--devices", "0,x"], "--devices wants a comma separated list of GPU ordinals, got '0,x'")
    # an error of the options' values comes before a missing owner, a missing owner before a missing input
    _dies(["--flank", "5", "--mask", "medium"], "--mask wants soft or hard, got 'medium'")
    _fails([], "ERROR: Please specify an input fasta file!\n")
    _fails(["--masked-fasta", tmp_path / "missing" / "out"], "ERROR: Please specify an input fasta file!\n")


def test_help_names_every_row_output_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert r.stderr.startswith("Below are the running options for the tool.:\n")
    for option in [o for o, _ in OUTPUTS] + [q for q, _, _ in QUALIFIERS]:
        assert f"\n  {option} arg " in r.stderr, option
    # help wins over everything that is checked after the options have been read
    assert subprocess.run([BIN, "-h", "--flank", "5"], capture_output=True, text=True, timeout=60).stderr == r.stderr
