"""The rows' CIGARs decoded without a GPU: ribbit_host_record_interruptions against the plain-Python statement of the contract
(tests/interruptions_contract.py), what follows from the contract, ribbit_bed_cigars, the two text functions byte for byte, every
refusal with its text, and ribbit-hip's handling of --interruption-bed and --purity-bed up to the point where it would touch a
GPU."""
import os
import subprocess

import numpy as np
import pytest

import interruptions_contract as ic
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
LENGTHS = (0, 1, 64, 300, 4100)
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed"]


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgtn", np.uint8)[np.random.RandomState(seed).randint(0, 10, n)].tobytes()


def check(sequence, intervals, ks, cigars, properties=True):
    got = ic.unpack(*ribbit_amd.host_record_interruptions(sequence, intervals, ks, cigars))
    want = ic.record_interruptions(sequence, intervals, cigars)
    assert got == want, cigars[:5]
    if properties:
        ic.check_properties(sequence, intervals, cigars, *want)
    return want


def test_host_twin_on_the_edge_sets():
    for length in LENGTHS:
        for iv, ks, cigars in ic.edge_case_sets(length):
            check(_seq(length, length), iv, ks, cigars)


def test_the_shapes_by_hand():
    seq = b"ACGTNacgtnACGTACGTAC"
    one = lambda s, c: check(seq, [(s, s + ic.query_of(c))], [2], [c])
    assert one(3, b"") == ([(0, 0, 0, 0, 0, 0, 3, 3)], [], [])
    assert one(3, b"5=") == ([(0, 0, 0, 0, 0, 5, 3, 8)], [], [])
    # a leading and a trailing non-match
    assert one(1, b"2X5=1I") == ([(0, 2, 2, 1, 0, 8, 3, 8)], [(0, 1, 3, 2, 0, 0, 0, 2), (0, 8, 9, 0, 1, 0, 4, 2)], [b"CG", b"t"])
    # all non-match: one interruption, no stretch
    assert one(4, b"2X1I3D") == ([(0, 1, 2, 1, 3, 3, 4, 4)], [(0, 4, 7, 2, 1, 3, 0, 6)], [b"Nac"])
    # = and M merge into one stretch
    assert one(0, b"3=2M4=") == ([(0, 0, 0, 0, 0, 9, 0, 9)], [], [])
    # two equal longest stretches: the leftmost
    assert one(2, b"3=1X3=1X2=")[0] == [(0, 2, 2, 0, 0, 10, 2, 5)]
    assert one(2, b"2=1X3=1X3=")[0] == [(0, 2, 2, 0, 0, 10, 5, 8)]
    # a D-only site has start == end and no observed bases
    assert one(5, b"2=3D2=") == ([(0, 1, 0, 0, 3, 4, 5, 7)], [(0, 7, 7, 0, 0, 3, 2, 2)], [b""])
    # ten digits
    assert one(0, b"2147483647=")[0] == [(0, 0, 0, 0, 0, 2147483647, 0, 2147483647)]
    assert one(-5, b"0000000003X2=") == ([(0, 1, 3, 0, 0, 5, -2, 0)], [(0, -5, -2, 3, 0, 0, 0, 11)], [b""])
    # rows one after the other: first is the prefix sum, cigar_at points into the pool
    rows, sites, observed = check(seq, [(0, 4), (4, 4), (2, 9)], [1, 2, 3], [b"1X2=1X", b"", b"3=1I1D3="])
    assert [r[:2] for r in rows] == [(0, 2), (2, 0), (2, 1)]
    assert sites == [(0, 0, 1, 1, 0, 0, 0, 2), (0, 3, 4, 1, 0, 0, 4, 2), (2, 5, 6, 0, 1, 1, 8, 4)] and observed == [b"A", b"T", b"a"]


def test_random_records():
    rs = np.random.RandomState(31)
    rows = sites = 0
    for t in range(60):
        sequence, iv, ks, cigars = ic.random_record(rs, t)
        got = check(sequence, iv, ks, cigars)
        rows += len(got[0])
        sites += len(got[1])
    assert rows > 2000 and sites > 5000


def test_bad_arguments():
    L = ribbit_amd.load_library()

    def refused(cigars, message, iv=None, ks=None, offsets=None, seq=b"ACGT" * 5):
        iv = [(0, 1)] * (len(cigars) if offsets is None else len(offsets) - 1) if iv is None else iv
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.host_record_interruptions(seq, iv, [1] * len(iv) if ks is None else ks, cigars, offsets)
        assert message in L.ribbit_hip_last_error().decode(), L.ribbit_hip_last_error().decode()

    refused([b"5=", b"3=1Y2="], "byte 5 (row 1) is neither a digit nor one of = M X I D")
    refused([b"5=", b"3=1x"], "byte 5 (row 1) is neither")
    refused([b"5 ="], "byte 1 (row 0) is neither")
    refused([b"=5"], "byte 0 (row 0) is an op letter without a length before it")
    refused([b"5==", b"1Y"], "byte 2 (row 0) is an op letter without")
    refused([b"", b"12345678901="], "byte 11 (row 1) ends an op of more than ten digits")
    refused([b"3=0X"], "byte 3 (row 0) ends an op whose length is not 1 .. 2147483647")
    refused([b"2147483648="], "byte 10 (row 0) ends an op whose length is not")
    refused([b"9999999999="], "byte 10 (row 0) ends an op whose length is not")
    refused([b"3=", b"12", b"3="], "byte 4 (row 1) is the row's end, behind digits without an op letter")
    refused([b"3=12"], "byte 4 (row 0) is the row's end")
    refused([b"2147483647=1D"], "row 0: the CIGAR's op lengths sum to 2147483648")
    refused([b"1=", b"2147483647="], "row 1: its start 1 and its CIGAR's query length 2147483647 do not fit int32", iv=[(0, 1), (1, 5)])
    refused([b"5="], "row 0: a motif of 0 bases", ks=[0])
    refused(b"5=3=", "offsets do not ascend", offsets=[0, 3, 2])
    refused(b"5=3=", "start at 1, not at 0", offsets=[1, 2, 4])
    refused(b"5=3=", "do not ascend", offsets=[0, 2, -(1 << 31)])
    # the first offending row decides, its grammar before its sums
    refused([b"2147483647=1D1Y", b"=1"], "byte 14 (row 0) is neither")
    ok = ribbit_amd.host_record_interruptions(b"", [((1 << 31) - 1 - 5, 0), (-(1 << 31), 0)], [1, 1], [b"5=", b"2147483646X1D"])
    assert ic.unpack(*ok)[0] == [(0, 0, 0, 0, 0, 5, (1 << 31) - 6, (1 << 31) - 1), (0, 1, 2147483646, 0, 1, 2147483646, -(1 << 31), -(1 << 31))]


def _line(name, s, e, motif, cigar):
    return f"{name}\t{s}\t{e}\t{motif}\t2|2\t7\t3.5\t0.9\t+\tP\t{cigar}\n"


def test_bed_cigars():
    cigars = ["5=", "", "3=1X3=1X5=1D82=", "1X" * 300, "7M"]
    bed = "".join(_line("a\tname with\ttabs", k, k + 5, "AC", c) for k, c in enumerate(cigars))
    for text in (bed, bed[:-1]):      # a last line without its newline counts
        pool, off = ribbit_amd.bed_cigars(text)
        assert pool == "".join(cigars).encode() and off.dtype == np.int32
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).tolist()
    pool, off = ribbit_amd.bed_cigars("")
    assert pool == b"" and off.tolist() == [0]
    # the grammar is not looked at here
    assert ribbit_amd.bed_cigars(_line("r", 1, 2, "AC", "what ever"))[0] == b"what ever"
    L = ribbit_amd.load_library()
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_cigars(_line("rec", 0, 5, "AC", "5=") + "rec\t1\t2\tAC\t5=\n")      # not a row of 11 columns
    assert f"at byte {len(_line('rec', 0, 5, 'AC', '5='))} " in L.ribbit_hip_last_error().decode()
    # a text large enough to be cut into parts
    rs = np.random.RandomState(3)
    shapes = [ic.random_cigar(rs, int(k)).decode() for k in rs.randint(0, 12, 500)]
    many = [shapes[i] for i in rs.randint(0, 500, 180_000)]
    big = "".join(_line("rec", k, k + 9, "ACG", c) for k, c in enumerate(many))
    assert len(big) > 8 << 20
    pool, off = ribbit_amd.bed_cigars(big)
    assert pool == "".join(many).encode() and np.array_equal(np.diff(off), [len(c) for c in many])


def test_the_two_texts_byte_for_byte():
    seq = b"ACGTNacgtnACGTACGTACGTTTTT"
    name = "rec\twith a tab"
    table = [(2, 12, "AC", "3=1X2I1D2=2M"),       # two stretches, the second the longer; one interruption of three ops
             (0, 5, "ACG", "5="),                  # pure
             (3, 3, "A", "2D"),                    # a D-only site: start == end, no observed bases
             (4, 20, "ACGT", "3=1X3=1X2="),        # inconsistent: the CIGAR spans 10 bases, the row 16
             (10, 19, "GT", "1X3=1I1D3=1X"),       # a leading and a trailing site; two equal stretches
             (-2, 1, "T", "3X"),                   # starts before the record
             (7, 7, "ACGTA", "")]                  # no CIGAR
    bed = "".join(_line(name, *row) for row in table)
    iv = ribbit_amd.bed_intervals(bed)
    pool, off = ribbit_amd.bed_cigars(bed)
    ks = [len(row[2]) for row in table]
    rows, sites, observed, obs_off = ribbit_amd.host_record_interruptions(seq, iv, ks, pool, off)
    want_sites = (f"{name}\t5\t8\t1X2I1D\tacg\t2\t12\tAC\t1\n"
                  f"{name}\t3\t3\t2D\t.\t3\t3\tA\t0\n"
                  f"{name}\t10\t11\t1X\tA\t10\t19\tGT\t0\n"
                  f"{name}\t14\t15\t1I1D\tA\t10\t19\tGT\t2\n"
                  f"{name}\t18\t19\t1X\tA\t10\t19\tGT\t4\n"
                  f"{name}\t-2\t1\t3X\tA\t-2\t1\tT\t0\n")
    assert ribbit_amd.interruption_text(name, bed, iv, rows, sites, pool, observed, obs_off) == (want_sites.encode(), 1)
    assert ribbit_amd.interruption_text(name, bed[:-1], iv, rows, sites, pool, observed, obs_off) == (want_sites.encode(), 1)
    extra = ["1\t1\t2\t1\t8\t12\t2", "0\t0\t0\t0\t0\t5\t1", "1\t0\t0\t2\t3\t3\t0", "2\t2\t0\t0\t.\t.\t.", "3\t2\t1\t1\t11\t14\t1", "1\t3\t0\t0\t-2\t-2\t0",
             "0\t0\t0\t0\t7\t7\t0"]
    want_rows = "".join(_line(name, *row)[:-1] + "\t" + more + "\n" for row, more in zip(table, extra))
    assert all(line.count("\t") == 17 + 1 for line in want_rows.splitlines())      # 18 columns, and the tab in the name
    assert ribbit_amd.bed_purity_text(bed, iv, ks, rows) == want_rows.encode()
    assert ribbit_amd.bed_purity_text(bed[:-1], iv, ks, rows) == want_rows.encode()
    none = ribbit_amd.host_record_interruptions(seq, [], [], [])
    assert ribbit_amd.interruption_text(name, "", [], *none[:2], b"", *none[2:]) == (b"", 0) and ribbit_amd.bed_purity_text("", [], [], none[0]) == b""
    # ---- every bad argument, with its text
    L = ribbit_amd.load_library()

    def refused(message, call):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            call()
        assert message in L.ribbit_hip_last_error().decode(), L.ribbit_hip_last_error().decode()

    refused("has 8 lines, not the 7", lambda: ribbit_amd.interruption_text(name, bed + "\n", iv, rows, sites, pool, observed, obs_off))
    refused("has 8 lines, not the 7", lambda: ribbit_amd.bed_purity_text(bed + "\n", iv, ks, rows))
    refused("row 2: a motif of 0 bases", lambda: ribbit_amd.bed_purity_text(bed, iv, [2, 3, 0, 4, 2, 1, 5], rows))
    bad = rows.copy()
    bad["count"][6] = 1
    refused("row 6: interruptions 8 .. 9 of 8", lambda: ribbit_amd.interruption_text(name, bed, iv, bad, sites, pool, observed, obs_off))
    bad = rows.copy()
    bad["first"][1] = -1
    refused("row 1: interruptions -1 .. -1 of 8", lambda: ribbit_amd.interruption_text(name, bed, iv, bad, sites, pool, observed, obs_off))
    bad = sites.copy()
    bad["row"][1] = 0
    refused("row 2: interruption 1 is row 0's", lambda: ribbit_amd.interruption_text(name, bed, iv, rows, bad, pool, observed, obs_off))
    bad = sites.copy()
    bad["cigar_at"][5] = len(pool) - 1
    refused(f"interruption 5: CIGAR bytes {len(pool) - 1} .. {len(pool) - 1 + int(sites['cigar_len'][5])} of a pool of {len(pool)}",
            lambda: ribbit_amd.interruption_text(name, bed, iv, rows, bad, pool, observed, obs_off))
    bad = sites.copy()
    bad["cigar_len"][0] = -1
    refused("interruption 0: CIGAR bytes", lambda: ribbit_amd.interruption_text(name, bed, iv, rows, bad, pool, observed, obs_off))
    refused("offsets start at 1, not at 0", lambda: ribbit_amd.interruption_text(name, bed, iv, rows, sites, pool, observed + b"A", obs_off + 1))
    bad = obs_off.copy()
    bad[2] = 1
    refused("interruption 1: the observed bases' offsets do not ascend", lambda: ribbit_amd.interruption_text(name, bed, iv, rows, sites, pool, observed, bad))
    refused("has 6 lines, not the 7", lambda: ribbit_amd.bed_purity_text("".join(_line(name, *row) for row in table[:6]), iv, ks, rows))
    refused("line 0 of the BED text is not a row", lambda: ribbit_amd.interruption_text(name, "r\t2\t12\n" + "".join(_line(name, *row) for row in table[1:]), iv, rows,
                                                                                         sites, pool, observed, obs_off))
    # a text large enough for the writers to work in pieces: CIGARs made long by zero-padded lengths, so that the rows stay few
    rs = np.random.RandomState(5)
    shapes = [ic.random_cigar(rs, int(k), b"=X=I=D") + b"0000000001=" * 15 for k in rs.randint(0, 9, 300)]
    spans = [ic.query_of(c) for c in shapes]
    pick = rs.randint(0, 300, 45_000).tolist()
    cigars = [shapes[i] for i in pick]
    big_iv = np.array([(3 * k, 3 * k + spans[i]) for k, i in enumerate(pick)])
    big = "".join(_line("rec", 3 * k, 3 * k + spans[i], "ACGTA"[:1 + k % 5], shapes[i].decode()) for k, i in enumerate(pick))
    assert len(big) > 2 << 22
    big_seq = _seq(int(big_iv[-1, 1]) + 10, 9)
    big_ks = [1 + k % 5 for k in range(len(cigars))]
    rows, sites, observed, obs_off = ribbit_amd.host_record_interruptions(big_seq, big_iv, big_ks, cigars)
    want = ic.unpack(rows, sites, observed, obs_off)      # (the decode is not what is tested here: the texts are, from the twin's arrays)
    pool = b"".join(cigars)
    text, left = ribbit_amd.interruption_text("rec", big, big_iv, rows, sites, pool, observed, obs_off)
    lo, hi = big_iv[:, 0].tolist(), big_iv[:, 1].tolist()
    assert left == 0 and text == "".join(
        f"rec\t{k[1]}\t{k[2]}\t{pool[k[6]:k[6] + k[7]].decode()}\t{o.decode() or '.'}\t{lo[k[0]]}\t{hi[k[0]]}\t{'ACGTA'[:big_ks[k[0]]]}\t"
        f"{(k[1] - lo[k[0]]) // big_ks[k[0]]}\n" for k, o in zip(want[1], want[2])).encode()
    lines = ribbit_amd.bed_purity_text(big, big_iv, big_ks, rows).decode().splitlines()
    assert lines == [row + "\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (r[1], r[2], r[3], r[4], r[6], r[7], (r[7] - r[6]) // k)
                     for row, r, k in zip(big.splitlines(), want[0], big_ks)]


# ---- ribbit-hip --interruption-bed / --purity-bed before the tool touches a GPU: exit status 1 and the exact text on stderr
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_cli_file_names():
    for option in ("--interruption-bed", "--purity-bed"):
        _dies([option + "="], f"{option} wants a file name")
        _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    _dies(["-i", "in.fa", "--purity-bed", "x", "--purity-units", "3"], "unrecognised option '--purity-units'")


@needs_tool
def test_cli_the_two_files_are_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\n")
    for option in ("--interruption-bed", "--purity-bed"):
        out = tmp_path / "missing" / "out"
        _dies(["-i", tmp_path / "in.fa", option, out], f"{option}: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + ["--interruption-bed", "--purity-bed"]
    for bad in (9, 10, 11):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]
    # neither needs --overlap-with, and an --overlap-with beside them alone still wants one of its own outputs
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", other, "--interruption-bed", tmp_path / "x", "--purity-bed", tmp_path / "y"],
          "--overlap-with needs --overlap-bed or --overlap-summary")
    assert not (tmp_path / "x").exists() and not (tmp_path / "y").exists()


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert "\n  --interruption-bed arg " in r.stderr and "\n  --purity-bed arg " in r.stderr
    assert r.stderr.index("--compound-gap arg") < r.stderr.index("--interruption-bed arg") < r.stderr.index("--purity-bed arg")
    assert "longest uninterrupted stretch" in r.stderr
