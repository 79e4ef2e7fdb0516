"""The best non-overlapping rows without a GPU: ribbit_host_record_best against the plain-Python statement of the contract
(tests/best_contract.py) and against a brute force over all subsets, what follows from the contract, ribbit_bed_rows_text, and
ribbit-hip's handling of --best-bed up to the point where it would touch a GPU."""
import os
import subprocess

import numpy as np
import pytest

import best_contract
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 2048, 4100)
OTHER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary"]


def check_best(length, intervals):
    rows, bases = ribbit_amd.host_record_best(length, intervals)
    assert rows.dtype == np.int32
    want_rows, want_bases = best_contract.record_best(length, intervals)
    assert (rows.tolist(), bases) == (want_rows, want_bases), length
    best_contract.check_properties(length, intervals, want_rows, want_bases)
    return want_rows, want_bases


def test_host_twin_on_the_edge_sets():
    for length in LENGTHS:
        for iv in best_contract.edge_case_sets(length):
            check_best(length, iv)
    # the whole record beside its parts: the parts tie with it and lose (the comparison is strict), one base more and they win
    assert check_best(100, [(0, 50), (50, 100), (0, 100)]) == ([2], 100)
    assert check_best(101, [(0, 50), (50, 101), (0, 100)]) == ([0, 1], 101)
    assert check_best(0, [(0, 5), (-3, 9)]) == ([], 0)


def test_host_twin_on_random_sets():
    rs = np.random.RandomState(77)
    selected = 0
    for t in range(300):
        length, iv = best_contract.random_record(rs, t)
        selected += len(check_best(length, iv)[0])
    assert selected > 3000


def test_no_subset_covers_more():
    rs = np.random.RandomState(5)
    for t in range(300):
        length = int(rs.randint(1, 80))
        n = int(rs.randint(0, 13))
        starts = rs.randint(-5, length + 5, n)
        iv = np.stack([starts, starts + rs.randint(-3, 30 if t % 2 else 8, n)], 1)
        _, bases = check_best(length, iv)
        assert bases == best_contract.brute_force_bases(length, iv), iv.tolist()


def test_ties_and_permutations():
    rows = [(100, 130), (90, 120), (110, 140), (95, 100), (300, 310), (301, 311), (299, 309), (302, 303)]
    rs = np.random.RandomState(3)
    chosen, bases = check_best(400, rows)
    want = [rows[i] for i in chosen]
    assert bases == 45
    for _ in range(20):
        shuffled = [rows[i] for i in rs.permutation(len(rows))]
        got, got_bases = check_best(400, shuffled)
        assert ([shuffled[i] for i in got], got_bases) == (want, bases)
    # among identical rows the lowest index
    assert check_best(400, [(20, 30)] * 5 + [(100, 130)] * 3) == ([0, 5], 40)
    assert check_best(400, [(100, 130)] * 3 + [(20, 30)] * 5) == ([3, 0], 40)
    # the same rows after clipping are identical rows too
    assert check_best(400, [(390, 900), (390, 400), (-7, 10), (0, 10)]) == ([2, 0], 20)
    # random sets: the selected (s', e') do not depend on the order the rows come in
    for t in range(50):
        length, iv = best_contract.random_record(rs, t)
        chosen, bases = check_best(length, iv)
        perm = rs.permutation(len(iv))
        again, again_bases = check_best(length, iv[perm])
        clipped, shuffled = best_contract.clipped(length, iv), best_contract.clipped(length, iv[perm])
        assert ([shuffled[i] for i in again], again_bases) == ([clipped[i] for i in chosen], bases)


def test_bad_arguments():
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.host_record_best(-1, [(0, 1)])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.host_record_best(1 << 31, [(0, 1)])
    assert check_best((1 << 31) - 1, [(-(1 << 31), (1 << 31) - 1)]) == ([0], (1 << 31) - 1)


def test_bed_rows_text():
    lines = [f"rec\t{10 * k}\t{10 * k + 7}\tAC\t2|2\t7\t3.5\t0.9{k}\t+\tP\t7=\n" for k in range(40)]
    bed = "".join(lines)
    for rows in ([], [0], [39], [3, 5, 4, 5], list(range(40)), list(range(39, -1, -1))):
        assert ribbit_amd.bed_rows_text(bed, rows) == "".join(lines[i] for i in rows).encode()
    # a last line without its newline is a line, and is written with one
    assert ribbit_amd.bed_rows_text(bed[:-1], [39, 0]) == (lines[39] + lines[0]).encode()
    assert ribbit_amd.bed_rows_text(bed[:-1], [38]) == lines[38].encode()
    # an index that is no line
    for text, rows in ((bed, [40]), (bed, [0, -1]), (bed[:-1], [40]), ("", [0]), (bed + "\n", [42])):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.bed_rows_text(text, rows)
    assert ribbit_amd.bed_rows_text(bed + "\n", [40]) == b"\n"      # (an empty line is a line)
    assert ribbit_amd.bed_rows_text("", []) == b""
    # a text and a selection large enough for the writer to work in pieces
    big = [f"rec\t{10 * k}\t{10 * k + 7}\tAC\t2|2\t7\t3.5\t0.9\t+\tP\t7=\n" for k in range(200_000)]
    many = np.random.RandomState(1).randint(0, len(big), 20_000).tolist()
    assert len("".join(big)) > 2 << 22
    assert ribbit_amd.bed_rows_text("".join(big), many) == "".join(big[i] for i in many).encode()
    # the selection of the host twin, as the tool writes it
    chosen, _ = ribbit_amd.host_record_best(1000, ribbit_amd.bed_intervals(bed))
    assert ribbit_amd.bed_rows_text(bed, chosen) == bed.encode()


# ---- ribbit-hip --best-bed before the tool touches a GPU: exit status 1 and the exact text on stderr
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_cli_file_name():
    _dies(["--best-bed="], "--best-bed wants a file name")
    _dies(["-i", "in.fa", "--best-bed", ""], "--best-bed wants a file name")
    _dies(["-i", "in.fa", "--best-bed"], "the required argument for option '--best-bed' is missing")
    _dies(["-i", "in.fa", "--best-bed", "x", "--best-gap", "3"], "unrecognised option '--best-gap'")


@needs_tool
def test_cli_best_bed_is_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\n")
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", "--best-bed", out], f"--best-bed: cannot open '{out}' for writing")
    options = OTHER_OUTPUTS + ["--best-bed"]
    for bad in (5, 6):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]
    # it needs no --overlap-with, and an --overlap-with beside it alone still wants one of its own outputs
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", other, "--best-bed", tmp_path / "x"], "--overlap-with needs --overlap-bed or --overlap-summary")
    assert not (tmp_path / "x").exists()


@needs_tool
def test_cli_help_names_the_option():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert "\n  --best-bed arg " in r.stderr
    assert r.stderr.index("--overlap-summary arg") < r.stderr.index("--best-bed arg")
    assert "no two overlap" in r.stderr
