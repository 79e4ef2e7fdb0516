"""ribbit-hip's argument handling for --overlap-with, --overlap-bed and --overlap-summary: every command line here ends in an
error message or the help text before the tool touches a GPU, so none of this needs one.  Exit status 1 and the exact text on
stderr."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
pytestmark = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")

OLD_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph"]
NEW_OUTPUTS = ["--overlap-bed", "--overlap-summary"]
INPUT_MISSING = "ERROR: Please specify an input fasta file!\n"


def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == message, args
    return r


def _dies(args, message):
    return _fails(args, "ribbit-hip: " + message + "\n")


def _cannot_open(option, path):
    return f"{option}: cannot open '{path}' for writing"


def _not_bed(k, path):
    return f"--overlap-with: line {k} of '{path}' is not a BED line (name, start, end)"


@pytest.fixture
def other(tmp_path):
    path = tmp_path / "other.bed"
    path.write_text("a\t1\t5\n")
    return path


def test_the_three_options_need_each_other(other):
    _dies(["--overlap-with", other], "--overlap-with needs --overlap-bed or --overlap-summary")
    _dies(["-i", "in.fa", f"--overlap-with={other}", "--loci-bed", "x"], "--overlap-with needs --overlap-bed or --overlap-summary")
    for option in NEW_OUTPUTS:
        _dies([option, "out"], f"{option} needs --overlap-with")
        _dies(["-i", "in.fa", f"{option}=out"], f"{option} needs --overlap-with")
    # both without their input: the first in the order of the outputs
    _dies(["--overlap-summary", "s", "--overlap-bed", "b"], "--overlap-bed needs --overlap-with")


@pytest.mark.parametrize("option", ["--overlap-with"] + NEW_OUTPUTS)
def test_empty_and_missing_file_names(option):
    _dies([option + "="], f"{option} wants a file name")
    _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
    _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")


def test_values_before_owners_before_the_missing_input(other, tmp_path):
    # a value error wins over a missing owner
    _dies(["--overlap-bed", "out", "--mask", "medium"], "--mask wants soft or hard, got 'medium'")
    _dies(["--overlap-with", other, "--density-window", "0"], "--density-window wants a whole number of bases (1 .. 2147483647), got '0'")
    # the qualifiers' owners are asked for first, as before, then the overlap options'
    _dies(["--overlap-bed", "out", "--flank", "5"], "--flank needs --repeat-fasta")
    # a missing owner wins over the missing input, the missing input over every file
    _dies(["--overlap-bed", tmp_path / "missing" / "out"], "--overlap-bed needs --overlap-with")
    _fails(["--overlap-with", tmp_path / "missing" / "other.bed", "--overlap-summary", tmp_path / "missing" / "out"], INPUT_MISSING)
    assert not (tmp_path / "missing").exists()


def test_unreadable_overlap_with_comes_before_any_output_file(tmp_path):
    missing = tmp_path / "nowhere" / "other.bed"
    paths = [tmp_path / f"out{k}" for k in range(7)]
    args = ["-i", tmp_path / "in.fa", "-o", paths[0], "--overlap-with", missing]
    for option, path in zip(OLD_OUTPUTS + NEW_OUTPUTS, paths[1:]):
        args += [option, path]
    _dies(args, f"--overlap-with: cannot open '{missing}' for reading")
    assert not any(p.exists() for p in paths)
    # ... and so does a line of it that is no BED line
    bad = tmp_path / "bad.bed"
    bad.write_text("a\t1\t5\nb\t7\n")
    args[args.index(missing)] = bad
    _dies(args, _not_bed(2, bad))
    assert not any(p.exists() for p in paths)


@pytest.mark.parametrize("text,line", [
    ("a\t1\n", 1),                                        # fewer than three columns
    ("a\n", 1),
    ("a 1 5\n", 1),                                       # blanks are no tabs
    ("a\t1\t5\n\n# note\ntrack name=x\nbrowser position a:1-5\nb\t2\n", 6),      # the skipped lines count as lines
    ("a\t1\t5\nb\tx\t9\n", 2),                            # no integers
    ("a\t1\t5\nb\t3\t9.0\n", 2),
    ("a\t1\t5\nb\t\t9\n", 2),
    ("a\t1\t5\nb\t3\t\n", 2),
    ("a\t1\t5\nb\t+3\t9\n", 2),
    ("a\t1\t5\nb\t3 \t9\n", 2),
    ("a\t1\t5\nb\t3\t2147483648\n", 2),                   # beyond int32, either way
    ("a\t1\t5\nb\t-2147483649\t9\n", 2),
    ("a\t1\t5\nb\t3\t99999999999999999999999\n", 2),
    ("a\t1\t5\nb\t3\t9\tmore\nc\t3", 3),                  # a last line without its newline is a line too
])
def test_malformed_lines_are_named_by_their_number(tmp_path, text, line):
    bed = tmp_path / "other.bed"
    bed.write_text(text)
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", bed, "--overlap-summary", tmp_path / "out"], _not_bed(line, bed))
    assert not (tmp_path / "out").exists()


def test_accepted_lines_reach_the_files(tmp_path):
    """what the reader takes: further columns, the int32 limits, reversed and negative intervals, a name with blanks, the skipped
    lines, no final newline -- the run then ends at the first output file that cannot be made"""
    bed = tmp_path / "other.bed"
    bed.write_text("# header\ntrack name=t\nbrowser hide all\n\na\t-2147483648\t2147483647\tACG\t3\nb c\t9\t2\nb c\t-5\t-1\n\na\t0\t0")
    out = tmp_path / "missing" / "out"
    for option in NEW_OUTPUTS:
        _dies(["-i", tmp_path / "in.fa", "--overlap-with", bed, option, out], _cannot_open(option, out))


def test_the_new_outputs_are_opened_after_the_old_ones(tmp_path, other):
    options = OLD_OUTPUTS + NEW_OUTPUTS
    for bad in range(len(options)):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, _cannot_open(options[bad], paths[bad]))
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", other, "--overlap-summary", out, "--overlap-bed", out], _cannot_open("--overlap-bed", out))


def test_help_names_the_three_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    for option in ["--overlap-with"] + NEW_OUTPUTS:
        assert f"\n  {option} arg " in r.stderr, option
    assert "not fractions" in r.stderr
    assert subprocess.run([BIN, "-h", "--overlap-bed", "x"], capture_output=True, text=True, timeout=60).stderr == r.stderr
