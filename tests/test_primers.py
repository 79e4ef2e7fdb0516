"""Primers in the flanks of chosen rows without a GPU: ribbit_host_record_primers against the plain statement of the contract
(tests/primers_contract.py), exactly; the text byte for byte against the plain formatter; every refusal with its text; and
ribbit-hip's handling of --primer-bed and --primer-flank up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import primers_contract as pc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed", "--nearest-bed", "--nearest-other-bed", "--composition-bed",
                   "--composition-track"]
# small oligos make every rule bite on short records: 5 .. 8 bases melt between 0 and 30 degrees
SMALL = dict(flank=30, min_length=5, max_length=8, opt_length=6, tm_min=0, tm_opt=150, tm_max=400, gc_min_percent=20, gc_max_percent=80)


def check(seq, rows, targets, what=None, loops=True, **fields):
    """the twin equals the contract, in both of its forms"""
    prm = pc.params(**fields)
    got = ribbit_amd.host_record_primers(seq, rows, targets, ribbit_amd.primer_params(**fields))
    assert got.dtype == ribbit_amd.PRIMERS_DT and got.shape == (len(targets),) and got.dtype.names == pc.FIELDS
    want = pc.record_primers_without_loops(seq, rows, targets, prm)
    assert pc.as_tuples(got) == want, (len(seq), what, fields)
    if loops:
        assert pc.record_primers(seq, rows, targets, prm) == want, (len(seq), what, fields)
    return want


def test_the_defaults_and_the_layout():
    p = ribbit_amd.primer_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == pc.DEFAULTS
    assert C.sizeof(p) == 44 and ribbit_amd.PRIMERS_DT.itemsize == 56 and len(pc.FIELDS) == 14
    assert ribbit_amd.primer_params(flank=7, gc_clamp=0).flank == 7
    with pytest.raises(TypeError):
        ribbit_amd.primer_params(flanks=7)


def test_the_tm_vectors():
    """the four oligos of the contract, in the table's own words and through the twin: an oligo as the only candidate of a right
    flank (its Tm admitted by a range of its own)"""
    for oligo, tm in pc.TM_VECTORS.items():
        assert pc.tm_of(oligo) == tm
        fields = dict(flank=20, min_length=20, max_length=20, opt_length=20, tm_min=0, tm_opt=tm, tm_max=2000, gc_min_percent=0, gc_max_percent=100, max_run=20, gc_clamp=0)
        seq = b"NNN" + oligo.encode().lower() + b"N"
        (row,) = check(seq, [], [(0, 3)], oligo, **fields)
        assert row == pc.NO_PRIMER + (3, 20, tm, 0) + row[10:12] + (0, 1)
        assert pc.oligo_of(row[6:12]) == oligo
        # the same bases as a left candidate: the Tm is the strand's own
        (row,) = check(seq, [], [(23, 24)], oligo, **fields)
        assert row[:4] == (3, 20, tm, 0) and row[12:] == (1, 0)


def test_by_hand():
    """a record of 40 bases whose flanks hold one candidate each, in the contract's words"""
    #       0         1         2         3
    #       0123456789012345678901234567890123456789
    seq = b"NNACGTGCANNNNNACACACACACNNNNNTGCATGGANNN"
    fields = dict(SMALL, min_length=7, max_length=7, opt_length=7, flank=13)
    (row,) = check(seq, [(14, 24)], [(14, 24)], **fields)
    left, right = row[:6], row[6:12]
    # left window [1, 14): ACGTGCA at 2 ends in A, every other start holds an N: with the clamp nothing is left
    assert left == pc.NO_PRIMER and row[12] == 0
    # right window [24, 37): TGCATGG at 29 starts with T (its 3' base on the reverse strand), GCATGGA at 30 starts with G
    assert right[:2] == (30, 7) and pc.oligo_of(right) == "GCATGGA" and row[13] == 1
    (row,) = check(seq, [(14, 24)], [(14, 24)], **dict(fields, gc_clamp=0))
    assert row[:2] == (2, 7) and row[12] == 1 and row[13] == 2
    text = ribbit_amd.bed_primers_text("r\t14\t24\tAC\n", ribbit_amd.host_record_primers(seq, [(14, 24)], [(14, 24)], ribbit_amd.primer_params(**dict(fields, gc_clamp=0))))
    tm_l, tm_r = pc.tm_of("ACGTGCA"), pc.tm_of("TGCATGG")
    # the nearer of the two right candidates wins only by penalty: both are 7 long, the Tm decides
    want_r = min((abs(pc.tm_of(o) - 150), d, o, s) for o, d, s in (("TGCATGG", 5, 29), ("GCATGGA", 6, 30)))
    rc = want_r[2][::-1].translate(pc.COMPLEMENT)
    assert text.decode() == f"r\t14\t24\tAC\t2\t9\tACGTGCA\t{pc.tenths(tm_l)}\t{want_r[3]}\t{want_r[3] + 7}\t{rc}\t{pc.tenths(pc.tm_of(want_r[2]))}\t{want_r[3] + 7 - 2}\t1\t2\n"
    assert tm_r == pc.tm_of("TGCATGG")


@pytest.mark.parametrize("length", (0, 1, 17, 64, 300))
def test_host_twin_on_the_edge_targets(length):
    for name, seq in (("random", pc.random_record(length, length)), ("clean", pc.clean_record(length, length)), ("all N", b"N" * length), ("one base", b"g" * length)):
        rows = [(5, 9), (40, 70), (length - 20, length + 5)]
        for flank in (0, 4, 30, 1000):
            want = check(seq, rows, pc.edge_targets(length), (name, flank), **dict(SMALL, flank=flank))
            if name in ("all N", "one base") or flank < 5:
                assert all(r[:6] == pc.NO_PRIMER and r[6:12] == pc.NO_PRIMER and r[12:] == (0, 0) for r in want)
    if length == 300:
        assert sum(r[0] >= 0 for r in check(pc.clean_record(300, 300), [], pc.edge_targets(300), **SMALL)) > 10


def test_the_defaults_on_random_records():
    rs = np.random.RandomState(11)
    for seed, seq in enumerate((pc.clean_record(3000, 1), pc.random_record(3000, 2), pc.random_record(2000, 3, b"ACGTacgtACGTacgtN"))):
        rows = pc.random_targets(len(seq), rs, 12, longest=40)
        targets = np.concatenate([rows[::2], pc.random_targets(len(seq), rs, 14)])
        want = check(seq, rows, targets, seed, loops=seed == 0)
        if seed != 1:
            assert sum(r[0] >= 0 and r[6] >= 0 for r in want) >= 5
        for (s, e), r in zip(targets.tolist(), want):
            s1, e1, lo, hi = pc.clip(s, e, 200, len(seq))
            assert r[0] == -1 or (lo <= r[0] and r[0] + r[1] <= s1 and 18 <= r[1] <= 25 and 570 <= r[2] <= 630 and r[12] >= 1)
            assert r[6] == -1 or (e1 <= r[6] and r[6] + r[7] <= hi and r[13] >= 1)


def test_flanks_partly_covered_by_other_rows():
    """a row inside a flank takes its bases away, whether or not it is a target; the target's own row never matters"""
    seq = pc.clean_record(400, 5)
    target = [(200, 220)]
    free = check(seq, target, target, **SMALL)[0]
    assert free[0] >= 0 and free[6] >= 0
    assert check(seq, [], target, **SMALL)[0] == free
    l_at, r_at = free[0], free[6]
    took = check(seq, target + [(l_at + 2, l_at + 3), (r_at, r_at + 1)], target, **SMALL)[0]
    assert took[0] != l_at and took[6] != r_at and took[12] < free[12] and took[13] < free[13]
    assert check(seq, [(150, 260)], target, **SMALL)[0] == pc.NO_PRIMER * 2 + (0, 0)
    # rows are clipped as the mask clips them: a reversed or outlying row covers nothing
    assert check(seq, [(260, 150), (-50, 0), (400, 500)], target, **SMALL)[0] == free


def test_non_default_parameters():
    seq = pc.clean_record(500, 9) + b"AAAAACCCCCGGGGGTTTTT" + pc.clean_record(100, 10)
    targets = [(100, 130), (300, 310), (505, 512), (0, 0), (620, 620)]
    for fields in (SMALL, dict(SMALL, gc_clamp=0), dict(SMALL, max_run=1), dict(SMALL, max_run=2), dict(SMALL, max_run=8), dict(SMALL, max_run=2**31 - 1),
                   dict(SMALL, tm_min=399, tm_opt=400, tm_max=400), dict(SMALL, gc_min_percent=50, gc_max_percent=50), dict(SMALL, gc_min_percent=0, gc_max_percent=0),
                   dict(SMALL, min_length=2, max_length=32, opt_length=17, tm_max=2000), dict(SMALL, min_length=32, max_length=32, opt_length=32, tm_max=2000, flank=40),
                   dict(flank=1000), dict(flank=17), dict(flank=18)):
        want = check(seq, [(100, 130)], targets, **fields)
        if fields.get("tm_min") == 399 or fields.get("flank") == 17:
            assert all(r[12:] == (0, 0) for r in want)
    # max_run 1 admits no two equal neighbours; the count shrinks, and with gc_clamp 0 it grows
    n = lambda **f: sum(r[12] + r[13] for r in check(seq, [], targets, loops=False, **dict(SMALL, **f)))
    assert n(max_run=1) < n(max_run=2) < n(max_run=8) == n(max_run=2**31 - 1) and n(gc_clamp=0) > n()


def test_the_tie_break():
    """two candidates with one penalty: the nearer one wins, on either side; of two at one distance the shorter"""
    unit = b"ACGTGCA"
    seq = unit * 6 + b"N" * 10 + unit * 6
    fields = dict(SMALL, min_length=7, max_length=7, opt_length=7, gc_clamp=0, flank=42)
    (row,) = check(seq, [], [(42, 52)], **fields)
    # every seventh start is the same oligo: the left winner ends nearest to 42, the right one starts nearest to 52
    by_oligo = {}
    for p in range(0, 36):
        by_oligo.setdefault(seq[p:p + 7], []).append(p)
    assert max(by_oligo[pc.oligo_of(row[:6]).encode()]) == row[0] and 52 + min(p for p in by_oligo[pc.oligo_of(row[6:12]).encode()]) == row[6]
    assert row[12] == row[13] == 36


def test_every_refusal():
    L = ribbit_amd.load_library()
    bad = [(dict(flank=-1), "flank -1 is outside 0 .. 1000"), (dict(flank=1001), "flank 1001 is outside 0 .. 1000"),
           (dict(max_length=33), "max_length 33 is above 32"), (dict(min_length=1), "min_length 1 is outside 2 .. max_length 25"),
           (dict(min_length=26), "min_length 26 is outside 2 .. max_length 25"), (dict(opt_length=17), "opt_length 17 is outside min_length 18 .. max_length 25"),
           (dict(opt_length=26), "opt_length 26 is outside min_length 18 .. max_length 25"), (dict(tm_max=2001), "tm_max 2001 is above 2000"),
           (dict(tm_opt=631), "tm_opt 631 is above tm_max 630"), (dict(tm_min=-1), "tm_min -1 is outside 0 .. tm_opt 600"),
           (dict(tm_min=601), "tm_min 601 is outside 0 .. tm_opt 600"), (dict(gc_max_percent=101), "gc_max_percent 101 is above 100"),
           (dict(gc_min_percent=-1), "gc_min_percent -1 is outside 0 .. gc_max_percent 60"), (dict(gc_min_percent=61), "gc_min_percent 61 is outside 0 .. gc_max_percent 60"),
           (dict(max_run=0), "max_run 0 is below 1"), (dict(gc_clamp=2), "gc_clamp 2 is neither 0 nor 1"), (dict(gc_clamp=-1), "gc_clamp -1 is neither 0 nor 1")]
    for fields, message in bad:
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: {message}$"):
            ribbit_amd.host_record_primers(b"ACGT", [], [(0, 1)], ribbit_amd.primer_params(**fields))
    # the limits themselves are accepted
    for fields in (dict(flank=0), dict(flank=1000), dict(min_length=2, opt_length=2, max_length=2), dict(max_length=32), dict(tm_min=0, tm_opt=0, tm_max=0),
                   dict(tm_opt=2000, tm_max=2000), dict(gc_min_percent=0, gc_max_percent=0), dict(gc_min_percent=100, gc_max_percent=100), dict(max_run=2**31 - 1)):
        assert len(ribbit_amd.host_record_primers(b"ACGT", [], [(0, 1)], ribbit_amd.primer_params(**fields))) == 1
    out, prm = C.c_void_p(), ribbit_amd.primer_params()
    iv = np.zeros(2, np.int32)
    assert L.ribbit_host_record_primers(b"ACGT", 4, None, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(out)) == -1
    assert L.ribbit_host_record_primers(b"ACGT", 4, iv.ctypes.data, 1, None, 1, C.byref(prm), C.byref(out)) == -1
    assert L.ribbit_host_record_primers(b"ACGT", 4, iv.ctypes.data, 1, iv.ctypes.data, 1, None, C.byref(out)) == -1
    assert L.ribbit_host_record_primers(b"ACGT", 4, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), None) == -1
    assert b"null argument" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_primers(None, 4, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(out)) == -1
    assert b"bad sequence" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_primers(b"ACGT", -1, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(out)) == -1
    assert L.ribbit_host_record_primers(b"ACGT", 2**31, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(out)) == -1
    assert b"a record of 2147483648 bases" in L.ribbit_hip_last_error()
    with pytest.raises(TypeError):
        ribbit_amd.host_record_primers(b"ACGT", [], [(0, 1)], pc.DEFAULTS)
    # no targets, no rows, no bases: no errors
    assert len(ribbit_amd.host_record_primers(b"ACGT", [(0, 2)], [])) == 0
    assert pc.as_tuples(ribbit_amd.host_record_primers(b"", [(0, 5)], [(0, 5), (-2, 2)])) == [pc.NO_PRIMER * 2 + (0, 0)] * 2
    assert L.ribbit_host_record_primers(None, 0, None, 0, None, 0, C.byref(prm), C.byref(out)) == 0
    L.ribbit_primers_free(out)
    L.ribbit_primer_params_default(None)


BED = "".join(f"rec one\t{s}\t{e}\tAC\t2\t{e - s}\t{(e - s) // 2}\t1.00\t+\tP\t{e - s}=\n" for s, e in ((60, 80), (0, 40), (290, 300), (150, 150)))


def test_the_text_byte_for_byte():
    seq = pc.clean_record(300, 3)
    rows = ribbit_amd.bed_intervals(BED).tolist()
    prm = ribbit_amd.primer_params(**SMALL)
    got = ribbit_amd.host_record_primers(seq, rows, rows, prm)
    want = pc.primer_lines(BED, pc.record_primers(seq, rows, rows, pc.params(**SMALL)))
    assert ribbit_amd.bed_primers_text(BED, got).decode() == want
    assert ribbit_amd.bed_primers_text(BED[:-1], got).decode() == want          # a last line without its newline counts
    lines = want.splitlines()
    assert all(len(line.split("\t")) == 22 and line.split("\t")[:11] == src.split("\t") for line, src in zip(lines, BED.splitlines()))
    # row 1 starts the record and row 2 ends it: one side each is missing, and so is the product
    assert lines[1].split("\t")[11:15] == ["."] * 4 and lines[1].split("\t")[19] == "." and lines[2].split("\t")[15:20] == ["."] * 5
    both = lines[0].split("\t")
    assert int(both[19]) == int(both[16]) - int(both[11]) and len(both[13]) == int(both[12]) - int(both[11]) and set(both[13] + both[17]) <= set("ACGT")
    assert seq[int(both[11]):int(both[12])].decode().upper() == both[13]
    assert seq[int(both[15]):int(both[16])].decode().upper() == both[17][::-1].translate(pc.COMPLEMENT)
    assert ribbit_amd.bed_primers_text("", got[:0]) == b""
    # the extreme values fit their columns
    big = np.array([(2**31 - 33, 32, 2000, 0, -1, -1, 2**31 - 33, 32, -15, 0, 0, 0, 2**31 - 1, 2**31 - 1)], dtype=ribbit_amd.PRIMERS_DT)
    assert ribbit_amd.bed_primers_text("x", big) == (b"x\t2147483615\t2147483647\t" + b"T" * 32 + b"\t200.0\t2147483615\t2147483647\t" + b"T" * 32
                                                      + b"\t-1.5\t32\t2147483647\t2147483647\n")
    assert ribbit_amd.bed_primers_text("x", big).decode() == pc.primer_lines("x", pc.as_tuples(big))


def test_every_refusal_of_the_text():
    L = ribbit_amd.load_library()
    got = ribbit_amd.host_record_primers(pc.clean_record(300, 3), [], ribbit_amd.bed_intervals(BED).tolist(), ribbit_amd.primer_params(**SMALL))
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 4 lines, not the 3 of the rows"):
        ribbit_amd.bed_primers_text(BED, got[:3])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 0 lines, not the 4 of the rows"):
        ribbit_amd.bed_primers_text("", got)
    for field, value in (("left_length", 0), ("left_length", 33), ("right_length", -1)):
        bad = got.copy()
        bad[field][0] = value
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: row 0: a primer of {value} bases, not 1 .. 32"):
            ribbit_amd.bed_primers_text(BED, bad)
    text, n = C.c_void_p(), C.c_size_t()
    assert L.ribbit_bed_primers_text(b"x", 1, None, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_primers_text(None, 1, got.ctypes.data, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_primers_text(b"x", 1, got.ctypes.data, 1, None, C.byref(n)) == -1
    assert L.ribbit_bed_primers_text(b"x", 1, got.ctypes.data, 1, C.byref(text), None) == -1
    assert b"null argument" in L.ribbit_hip_last_error()


def test_text_written_in_pieces():
    """a text large enough to be written by several threads (bed_text.h: a piece per 4 MB): the pieces meet where they should"""
    n = 250_000
    bed = "".join(f"r\t{k}\t{k + 9}\tACG\t3\t9\t3\t1.00\t+\tP\t9=\n" for k in range(n))
    assert len(bed) > 2 * (4 << 20)
    rs = np.random.RandomState(4)
    rows = rs.randint(-2**31, 2**31, (n, 14)).astype("<i4")
    rows[:, (1, 7)] = rs.randint(1, 33, (n, 2))
    rows[:, (0, 6)] = rs.randint(-1, 2**30, (n, 2))
    got = ribbit_amd.bed_primers_text(bed, rows.view(ribbit_amd.PRIMERS_DT).reshape(-1)).decode()
    assert got == pc.primer_lines(bed, rows.tolist())


# ---- the command-line tool, up to the GPU
def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == message, args


def _dies(args, message):
    _fails(args, "ribbit-hip: " + message + "\n")


@needs_tool
def test_cli_the_qualifier_needs_its_output(tmp_path):
    _dies(["--primer-flank", "5"], "--primer-flank needs --primer-bed")
    _dies(["-i", "in.fa", "--primer-flank=5"], "--primer-flank needs --primer-bed")
    # it belongs to its own output, not to the ones it quotes or resembles
    _dies(["--primer-flank", "5", "--best-bed", "b"], "--primer-flank needs --primer-bed")
    _dies(["--primer-flank", "5", "--composition-bed", "b", "--repeat-fasta", "r"], "--primer-flank needs --primer-bed")
    _dies(["--flank", "5", "--primer-bed", "b"], "--flank needs --repeat-fasta")
    _dies(["--composition-flank", "5", "--primer-bed", "b"], "--composition-flank needs --composition-bed")
    # the first in the order of the seventeen
    _dies(["--primer-flank", "5", "--composition-window", "5"], "--composition-window needs --composition-track")
    # with its output it is accepted, and --primer-bed needs no --best-bed: the next complaint is the missing input
    _fails(["--primer-bed", tmp_path / "missing" / "out", "--primer-flank", "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("1001", "-1", "x", "10000", "00000", "1e3", "", "5 ", "+5"):
        _dies(["-i", "in.fa", "--primer-bed", "b", "--primer-flank", value], f"--primer-flank wants a whole number of bases (0 .. 1000), got '{value}'")
    # accepted: the run then ends at the output file that cannot be made
    for value in ("0", "1000", "0200", "18"):
        _dies(["-i", tmp_path / "in.fa", "--primer-bed", out, "--primer-flank", value], f"--primer-bed: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--primer-bed", "b", "--primer-flank"], "the required argument for option '--primer-flank' is missing")


@needs_tool
def test_cli_file_names():
    _dies(["--primer-bed="], "--primer-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-bed", ""], "--primer-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-bed"], "the required argument for option '--primer-bed' is missing")
    _dies(["-i", "in.fa", "--primer-bed", "x", "--primer-gap", "3"], "unrecognised option '--primer-gap'")


@needs_tool
def test_cli_the_file_is_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", "--primer-bed", out], f"--primer-bed: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + ["--primer-bed"]
    assert len(options) == 17
    for bad in (15, 16):
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
    names = ["--composition-window", "--primer-bed", "--primer-flank"]
    for name in names:
        assert f"\n  {name} arg " in r.stderr
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[0]:at[1]].endswith("Default: 10000") and r.stderr[at[2]:].rstrip("\n").endswith("Default: 200")
    assert "check_primers" in r.stderr[at[1]:at[2]]
