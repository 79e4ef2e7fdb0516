"""The base composition of rows, flanks and windows without a GPU: ribbit_host_record_composition and
ribbit_host_record_base_windows against the plain statement of the contract (tests/composition_contract.py), the two text functions
byte for byte against the plain formatters, every refusal with its text, and ribbit-hip's handling of --composition-bed,
--composition-flank, --composition-track and --composition-window up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import composition_contract as cc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
B = cc.B
LENGTHS = (0, 1, 33, B - 1, B, B + 1, 2 * B + 1, 4095, 4096, 4097, 9000)      # word and block edges (the twin samples its prefix every 256 bases too), page edges
FLANKS = (0, 1, 31, 32, B - 1, B, 1000, 2**31 - 1)
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed", "--nearest-bed", "--nearest-other-bed"]
NEW_OUTPUTS = ["--composition-bed", "--composition-track"]
QUALIFIERS = {"--composition-bed": "--composition-flank", "--composition-track": "--composition-window"}


def _seq(n, seed=0):
    return next(cc.sequences(n, seed))[1]


def check_rows(seq, rows, flank, what=None):
    got = ribbit_amd.host_record_composition(seq, rows, flank)
    assert got.dtype == ribbit_amd.COMPOSITION_DT and got.shape == (len(rows),) and got.dtype.names == cc.FIELDS
    want = cc.record_composition(seq, rows, flank)
    assert cc.as_tuples(got) == want, (len(seq), flank, what)
    assert cc.record_composition_without_loops(seq, rows, flank).tolist() == [list(r) for r in want], (len(seq), flank, what)
    return want


def check_windows(seq, window):
    got = ribbit_amd.host_record_base_windows(seq, window)
    assert got.dtype == ribbit_amd.BASE_COUNTS_DT and got.shape == (-(-len(seq) // window),)
    want = cc.record_base_windows(seq, window)
    assert cc.as_tuples(got) == want, (len(seq), window)
    assert cc.record_base_windows_without_loops(seq, window).tolist() == [list(w) for w in want], (len(seq), window)
    return want


def test_the_rule_for_a_byte():
    """all 256 bytes: A, C, G, T in either case and nothing else, as the pack kernel folds them (c | 0x20)"""
    every = bytes(range(256))
    assert [cc.kind(b) for b in b"ACGTacgtNn-RY\x00\x01\x21\x41\x61"] == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 0, 0]
    for b in range(256):
        want = [0] * 5
        want[cc.kind(b)] = 1
        assert cc.counts(every, b, b + 1) == want
    assert cc.as_tuples(ribbit_amd.host_record_base_windows(every, 1)) == [tuple(cc.counts(every, b, b + 1)) for b in range(256)]
    assert cc.as_tuples(ribbit_amd.host_record_base_windows(every, 256)) == [(2, 2, 2, 2, 248)]


@pytest.mark.parametrize("length", LENGTHS)
def test_host_twin_on_the_edge_sets(length):
    seq = _seq(length, length)
    for what, rows in cc.edge_case_sets(length):
        for flank in FLANKS:
            check_rows(seq, rows, flank, what)


def test_the_shapes_by_hand():
    """the words of the contract on a record of 20 bases"""
    seq = b"AAACCGGTTTNNacgtRYAC"
    rows = [(3, 7), (0, 3), (10, 12), (18, 25), (-4, 2), (9, 9), (30, 40), (7, 3)]
    got = cc.as_tuples(ribbit_amd.host_record_composition(seq, rows, 4))
    assert got == [
        (0, 2, 2, 0, 0, 3, 0, 0, 3, 4, 0, 1, 1),      # CCGG; left AAA, all of it row 1's; right TTTN, the N being row 2's
        (3, 0, 0, 0, 0, 0, 0, 0, 0, 4, 4, 0, 4),      # at the record's start: no left flank; right CCGG, all of it row 0's
        (0, 0, 0, 0, 2, 4, 1, 0, 1, 4, 2, 0, 0),      # NN; left GTTT, the G being row 0's; right acgt counts as ACGT
        (1, 1, 0, 0, 0, 4, 1, 2, 0, 0, 0, 0, 0),      # clipped to 18 .. 20: AC; left gtRY; no right flank at the record's end
        (2, 0, 0, 0, 0, 0, 0, 0, 0, 4, 3, 0, 4),      # clipped to 0 .. 2; right ACCG
        (0, 0, 0, 0, 0, 4, 2, 0, 2, 4, 0, 2, 2),      # an empty row still has flanks: GGTT | TNNa
        (0, 0, 0, 0, 0, 4, 1, 2, 2, 0, 0, 0, 0),      # behind the end: s' = e' = 20; left RYAC, of which AC is row 3's
        (0, 0, 0, 0, 0, 4, 4, 0, 4, 4, 0, 1, 1),      # reversed: empty at s' = 7; left CCGG, right TTTN
    ]
    assert got == cc.record_composition(seq, rows, 4)
    assert cc.as_tuples(ribbit_amd.host_record_base_windows(seq, 8)) == [(3, 2, 2, 1, 0), (1, 1, 1, 3, 2), (1, 1, 0, 0, 2)]


@pytest.mark.parametrize("length", (1, 1000, 9000))
def test_random_sets(length):
    rs = np.random.RandomState(500 + length)
    for n in (1, 2, 300):
        seq = _seq(length, n)
        for flank in (0, 7, 100, 5000):
            want = check_rows(seq, cc.random_rows(length, rs, n, 60 if n % 2 else 2000), flank)
            for r in want:
                assert sum(r[:5]) <= length and r[6] + r[7] <= r[5] <= flank and r[10] + r[11] <= r[9] <= flank and r[8] <= r[5] and r[12] <= r[9]


@pytest.mark.parametrize("length", LENGTHS)
def test_windows(length):
    seq = _seq(length, 7 + length)
    whole = tuple(cc.counts(seq, 0, length))
    for window in sorted({w for w in (1, 31, 32, 33, B - 1, B, B + 1, length - 1, length, length + 1, 2**31 - 1) if w >= 1}):
        want = check_windows(seq, window)
        assert tuple(map(sum, zip(*want))) == (whole if length else ())


def test_sequences_that_end_in_other_bytes():
    """all N, one base throughout, a last N, an N run across a block edge: what lies behind the record's end is never counted"""
    for length in (0, 1, 33, B + 1, 2 * B + 1):
        for what, seq in cc.sequences(length):
            assert len(seq) == length
            for flank in (0, 3, 2**31 - 1):
                check_rows(seq, [(0, length), (length - 1, length + 3), (B - 3, B + 3), (length, length)], flank, what)
            check_windows(seq, 1 if length < 100 else 32)


def test_bad_arguments():
    L = ribbit_amd.load_library()
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: flank -1 is negative"):
        ribbit_amd.host_record_composition(b"ACGT", [(0, 1)], -1)
    for window in (0, -5):
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: window {window} is below 1"):
            ribbit_amd.host_record_base_windows(b"ACGT", window)
    with pytest.raises(ValueError):
        ribbit_amd.host_record_composition(b"ACGT", [(0, 1)], 2**31)
    out, n = C.c_void_p(), C.c_size_t()
    iv = np.zeros(2, np.int32)
    assert L.ribbit_host_record_composition(b"ACGT", 4, None, 1, 0, C.byref(out)) == -1
    assert L.ribbit_host_record_composition(b"ACGT", 4, iv.ctypes.data, 1, 0, None) == -1
    assert L.ribbit_host_record_composition(None, 4, iv.ctypes.data, 1, 0, C.byref(out)) == -1
    assert L.ribbit_host_record_composition(b"ACGT", -1, iv.ctypes.data, 1, 0, C.byref(out)) == -1
    assert L.ribbit_host_record_composition(b"ACGT", 2**31, iv.ctypes.data, 1, 0, C.byref(out)) == -1
    assert b"a record of 2147483648 bases" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_base_windows(None, 4, 1, C.byref(out), C.byref(n)) == -1
    assert L.ribbit_host_record_base_windows(b"ACGT", 4, 1, None, C.byref(n)) == -1
    assert L.ribbit_host_record_base_windows(b"ACGT", 4, 1, C.byref(out), None) == -1
    assert L.ribbit_host_record_base_windows(b"ACGT", -1, 1, C.byref(out), C.byref(n)) == -1
    # no rows, no bases: no errors
    assert len(ribbit_amd.host_record_composition(b"", [], 5)) == 0
    assert cc.as_tuples(ribbit_amd.host_record_composition(b"", [(0, 5), (-2, 2)], 5)) == [(0,) * 13] * 2
    assert len(ribbit_amd.host_record_base_windows(b"", 10)) == 0
    assert L.ribbit_host_record_composition(None, 0, None, 0, 0, C.byref(out)) == 0
    L.ribbit_composition_free(out)


BED = "".join(f"rec one\t{s}\t{e}\tAC\t2\t{e - s}\t{(e - s) // 2}\t1.00\t+\tP\t{e - s}=\n" for s, e in ((3, 9), (0, 40), (35, 50), (50, 50)))


def test_the_two_texts_byte_for_byte():
    seq = _seq(60, 3)
    rows = ribbit_amd.bed_intervals(BED).tolist()
    comp = ribbit_amd.host_record_composition(seq, rows, 10)
    want = cc.composition_lines(BED, cc.record_composition(seq, rows, 10))
    assert ribbit_amd.bed_composition_text(BED, comp).decode() == want
    assert ribbit_amd.bed_composition_text(BED[:-1], comp).decode() == want          # a last line without its newline counts
    assert all(len(line.split("\t")) == 24 and line.split("\t")[:11] == src.split("\t") for line, src in zip(want.splitlines(), BED.splitlines()))
    assert ribbit_amd.bed_composition_text("", comp[:0]) == b""
    for length, window in ((60, 7), (60, 60), (60, 61), (60, 1), (1, 1), (0, 5)):
        wins = ribbit_amd.host_record_base_windows(seq[:length], window)
        text = ribbit_amd.base_windows_text("rec one", length, window, wins).decode()
        assert text == cc.window_lines("rec one", length, window, cc.record_base_windows(seq[:length], window))
        assert len(text.splitlines()) == -(-length // window) and all(len(line.split("\t")) == 8 for line in text.splitlines())
    # the extreme values fit their columns
    big = np.full(1, 2**31 - 1, dtype="<i4").repeat(13).view(ribbit_amd.COMPOSITION_DT)
    assert ribbit_amd.bed_composition_text("x", big) == b"x" + b"\t2147483647" * 13 + b"\n"
    one = np.array([(2**31 - 1, 0, 0, 0, 0)], dtype=ribbit_amd.BASE_COUNTS_DT)
    assert ribbit_amd.base_windows_text("", 2**31 - 1, 2**31 - 1, one) == b"\t0\t2147483647\t2147483647\t0\t0\t0\t0\n"


def test_every_refusal_of_the_texts():
    L = ribbit_amd.load_library()
    comp = ribbit_amd.host_record_composition(_seq(60), ribbit_amd.bed_intervals(BED).tolist(), 10)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 4 lines, not the 3 of the rows"):
        ribbit_amd.bed_composition_text(BED, comp[:3])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 0 lines, not the 4 of the rows"):
        ribbit_amd.bed_composition_text("", comp)
    wins = ribbit_amd.host_record_base_windows(_seq(60), 7)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: 9 windows, not the 10 of a record of 64 bases in windows of 7"):
        ribbit_amd.base_windows_text("r", 64, 7, wins)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: 9 windows, not the 0 of a record of 0 bases in windows of 7"):
        ribbit_amd.base_windows_text("r", 0, 7, wins)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: window 0 is below 1"):
        ribbit_amd.base_windows_text("r", 60, 0, wins)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: a record of -1 bases"):
        ribbit_amd.base_windows_text("r", -1, 7, wins)
    with pytest.raises(ValueError):
        ribbit_amd.base_windows_text("r\0", 60, 7, wins)
    text, n = C.c_void_p(), C.c_size_t()
    assert L.ribbit_bed_composition_text(b"x", 1, None, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_composition_text(None, 1, comp.ctypes.data, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_composition_text(b"x", 1, comp.ctypes.data, 1, None, C.byref(n)) == -1
    assert L.ribbit_base_windows_text(None, 60, 7, wins.ctypes.data, 9, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_base_windows_text(b"r", 60, 7, None, 9, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_base_windows_text(b"r", 60, 7, wins.ctypes.data, 9, C.byref(text), None) == -1
    assert b"null argument" in L.ribbit_hip_last_error()


def test_texts_written_in_pieces():
    """texts large enough to be written by several threads (bed_text.h: a piece per 4 MB): the pieces meet where they should"""
    n = 250_000
    bed = "".join(f"r\t{k}\t{k + 9}\tACG\t3\t9\t3\t1.00\t+\tP\t9=\n" for k in range(n))
    assert len(bed) > 2 * (4 << 20)
    rs = np.random.RandomState(4)
    comp = rs.randint(0, 2**31, (n, 13)).astype("<i4")
    got = ribbit_amd.bed_composition_text(bed, comp.view(ribbit_amd.COMPOSITION_DT).reshape(-1)).decode()
    assert got == cc.composition_lines(bed, comp.tolist())
    m = 400_000
    wins = rs.randint(0, 2**31, (m, 5)).astype("<i4")
    got = ribbit_amd.base_windows_text("a long name", 3 * m - 1, 3, wins.view(ribbit_amd.BASE_COUNTS_DT).reshape(-1)).decode()
    assert got == cc.window_lines("a long name", 3 * m - 1, 3, wins.tolist())


# ---- the command-line tool, up to the GPU
def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == message, args


def _dies(args, message):
    _fails(args, "ribbit-hip: " + message + "\n")


@needs_tool
def test_cli_the_qualifiers_need_their_outputs(tmp_path):
    _dies(["--composition-flank", "5"], "--composition-flank needs --composition-bed")
    _dies(["-i", "in.fa", "--composition-window=5"], "--composition-window needs --composition-track")
    # each belongs to its own output, not to the other one or to the outputs whose qualifiers they resemble
    _dies(["--composition-flank", "5", "--composition-track", "t"], "--composition-flank needs --composition-bed")
    _dies(["--composition-window", "5", "--composition-bed", "b"], "--composition-window needs --composition-track")
    _dies(["--composition-flank", "5", "--repeat-fasta", "r"], "--composition-flank needs --composition-bed")
    _dies(["--composition-window", "5", "--density-bedgraph", "d"], "--composition-window needs --composition-track")
    _dies(["--flank", "5", "--composition-bed", "b"], "--flank needs --repeat-fasta")
    _dies(["--density-window", "5", "--composition-track", "t"], "--density-window needs --density-bedgraph")
    # the first in the order of the sixteen
    _dies(["--composition-window", "5", "--composition-flank", "5"], "--composition-flank needs --composition-bed")
    _dies(["--composition-flank", "5", "--loci-gap", "5"], "--loci-gap needs --loci-bed")
    # with their outputs they are accepted: the next complaint is the missing input
    for option in NEW_OUTPUTS:
        _fails([option, tmp_path / "missing" / "out", QUALIFIERS[option], "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("-1", "1000000000", "0000000000", "1e3", "", "5 ", "+5"):
        _dies(["-i", "in.fa", "--composition-bed", "b", "--composition-flank", value],
              f"--composition-flank wants a whole number of bases (0 or more, at most 9 digits), got '{value}'")
    for value in ("0", "-1", "2147483648", "00000000001", "1e3", "", "w"):
        _dies(["-i", "in.fa", "--composition-track", "t", f"--composition-window={value}"],
              f"--composition-window wants a whole number of bases (1 .. 2147483647), got '{value}'")
    # accepted: the run then ends at the output file that cannot be made
    for value in ("0", "999999999", "000000007"):
        _dies(["-i", tmp_path / "in.fa", "--composition-bed", out, "--composition-flank", value], f"--composition-bed: cannot open '{out}' for writing")
    for value in ("1", "2147483647", "0000000001"):
        _dies(["-i", tmp_path / "in.fa", "--composition-track", out, "--composition-window", value], f"--composition-track: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--composition-bed", "b", "--composition-flank"], "the required argument for option '--composition-flank' is missing")


@needs_tool
def test_cli_file_names():
    for option in NEW_OUTPUTS:
        _dies([option + "="], f"{option} wants a file name")
        _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    _dies(["-i", "in.fa", "--composition-bed", "x", "--composition-gap", "3"], "unrecognised option '--composition-gap'")


@needs_tool
def test_cli_the_two_files_are_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    for option in NEW_OUTPUTS:
        out = tmp_path / "missing" / "out"
        _dies(["-i", tmp_path / "in.fa", option, out], f"{option}: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + NEW_OUTPUTS
    for bad in (13, 14, 15):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    names = ["--nearest-other-bed", "--composition-bed", "--composition-flank", "--composition-track", "--composition-window"]
    for name in names:
        assert f"\n  {name} arg " in r.stderr
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[2]:at[3]].endswith("Default: 100") and "Default: 10000\n" in r.stderr[at[4]:]
