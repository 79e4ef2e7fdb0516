"""The rows by canonical motif class without a GPU: ribbit_host_record_classes against the plain-Python statement of the contract
(tests/classes_contract.py), what follows from the contract, ribbit_bed_motifs, the two text functions byte for byte, and
ribbit-hip's handling of --class-bed and --motif-summary up to the point where it would touch a GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import classes_contract as cc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
LENGTHS = (0, 1, 64, 300, 4100)
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed"]


def unpack(motifs, classes, strands, groups):
    """the library's result in the contract's form"""
    off = np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).astype(int)
    assert len(classes) == off[-1] and len(strands) == len(motifs)
    per_row = [classes[off[i]:off[i + 1]].decode() for i in range(len(motifs))]
    return per_row, list(strands.decode()), [(per_row[g["first_row"]], int(g["length"]), int(g["rows"]), int(g["bases"]), int(g["first_row"]), int(g["longest_row"]))
                                             for g in groups]


def check_classes(length, intervals, motifs, properties=True):
    got = unpack(motifs, *ribbit_amd.host_record_classes(length, intervals, motifs))
    want = cc.record_classes(length, intervals, motifs)
    assert got == want, (length, motifs[:5])
    if properties:
        cc.check_properties(length, intervals, motifs, *want)
    return want


def test_every_motif_up_to_six_bases():
    counts = []
    for k in range(1, 7):
        motifs = ["".join(t) for t in itertools.product("ACGT", repeat=k)]
        classes, strands, groups = check_classes(100, [(i % 90, i % 90 + 5) for i in range(len(motifs))], motifs)
        assert len(groups) == len({cc.motif_class(u)[0] for u in motifs})
        counts.append(len(groups))
    # the counts come from the contract (the line above), not from a table: they are 2, 6, 12, 39, 104, 366.  (2, 4, 10, 33, 102, 350
    # would be the classes with k as their least period; a class here keeps its length, so AA and ACAC count at k = 2 and 4.)
    print("classes of the motifs of 1 .. 6 bases:", counts)
    assert counts[0] == 2 and all(a < b for a, b in zip(counts, counts[1:]))


def test_host_twin_on_the_edge_sets():
    for length in LENGTHS:
        for iv, motifs in cc.edge_case_sets(length):
            check_classes(length, iv, motifs)
    assert check_classes(50, [(0, 9)], ["T"])[:2] == (["A"], ["-"])
    assert check_classes(50, [(0, 9), (1, 2), (3, 4)], ["AT", "ACGT", "AATT"])[1] == ["+"] * 3
    assert check_classes(50, [(0, 9)] * 3, ["ACAC", "ACGACG", cc.periodic("CGA", 990)])[0] == ["ACAC", "ACGACG", cc.periodic("ACG", 990)]
    # ties of the longest row go to the lowest index; empty and out-of-range rows are rows of 0 bases
    groups = check_classes(100, [(50, 40), (10, 20), (30, 40), (5, 15), (200, 300), (-9, -1)], ["CA", "AC", "TG", "GT", "AC", "AG"])[2]
    assert groups == [("AC", 2, 5, 30, 0, 1), ("AG", 2, 1, 0, 5, 5)]
    assert check_classes(0, [(0, 10), (3, 4)], ["GT", "CA"])[2] == [("AC", 2, 2, 0, 0, 0)]
    assert check_classes(100, [], []) == ([], [], [])


def test_random_motifs_at_every_length():
    rs = np.random.RandomState(21)
    for k in cc.MOTIF_LENGTHS:
        motifs = [cc.random_motif(rs, k) for _ in range(6)] + [cc.random_motif(rs, k, "AC") for _ in range(3)]
        motifs += [cc.reverse_complement(u[k // 3:] + u[:k // 3]) for u in motifs[:3]]
        classes, strands, groups = check_classes(5000, [(7 * i, 7 * i + 30) for i in range(len(motifs))], motifs)
        assert classes[9:12] == classes[:3]


def test_equal_keys_are_parted_by_the_bytes_behind_them():
    rs = np.random.RandomState(8)
    for k in (28, 33, 64, 500, 1023):
        twins = cc.key_twins(rs, k)
        classes, strands, groups = check_classes(1000, [(i, i + 10) for i in range(4)], twins)
        assert classes == twins and strands == ["+"] * 4 and len({c[:27] for c in classes}) == 1
        assert [g[0] for g in groups] == sorted(set(twins)) and sorted(g[2] for g in groups) == ([1, 1, 2] if k > 28 else [2, 2])


def test_random_records_and_their_shuffles():
    rs = np.random.RandomState(77)
    rows = 0
    for t in range(60):
        length, iv, motifs = cc.random_record(rs, t)
        classes, strands, groups = check_classes(length, iv, motifs)
        rows += len(motifs)
        # shuffling the rows changes no group's (class, length, rows, bases) and no row's (class, strand)
        perm = rs.permutation(len(motifs))
        again = check_classes(length, iv[perm], [motifs[i] for i in perm], properties=False)
        assert [g[:4] for g in again[2]] == [g[:4] for g in groups]
        assert (again[0], again[1]) == ([classes[i] for i in perm], [strands[i] for i in perm])
    assert rows > 2000


def test_bad_arguments():
    L = ribbit_amd.load_library()
    for motifs, message in ((["AC", ""], "an empty motif"), (["AC", "ACN"], "outside ACGT"), (["ac"], "outside ACGT"), (["A" * 1024], "1024 bytes")):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.host_record_classes(100, [(0, 1)] * len(motifs), motifs)
        assert message in L.ribbit_hip_last_error().decode()
    for offsets, message in (([0, 2, 1], "do not ascend"), ([1, 2, 4], "not at 0"), ([0, 2, -(1 << 31)], "do not ascend")):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.host_record_classes(100, [(0, 1), (0, 1)], b"ACGT", offsets)
        assert message in L.ribbit_hip_last_error().decode()
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.host_record_classes(-1, [(0, 1)], ["AC"])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.host_record_classes(1 << 31, [(0, 1)], ["AC"])
    assert check_classes((1 << 31) - 1, [(-(1 << 31), (1 << 31) - 1)] * 3, ["AC"] * 3)[2] == [("AC", 2, 3, 3 * ((1 << 31) - 1), 0, 0)]
    assert check_classes(100, [(0, 5)], ["A" * 1023])[0] == ["A" * 1023]


def _line(name, k, motif):
    return f"{name}\t{10 * k}\t{10 * k + 7}\t{motif}\t2|2\t7\t3.5\t0.9\t+\tP\t7=\n"


def test_bed_motifs():
    motifs = ["AC", "GATA", "T", "ACGT" * 200, "TG"]
    bed = "".join(_line("a\tname with\ttabs", k, m) for k, m in enumerate(motifs))
    for text in (bed, bed[:-1]):      # a last line without its newline counts
        pool, off = ribbit_amd.bed_motifs(text)
        assert pool == "".join(motifs).encode() and off.dtype == np.int32
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).tolist()
    pool, off = ribbit_amd.bed_motifs("")
    assert pool == b"" and off.tolist() == [0]
    L = ribbit_amd.load_library()
    for bad in ("ACN", "", "ac", "A" * 1024, "A C"):
        text = _line("rec", 0, "AC") + _line("rec", 1, bad) + _line("rec", 2, "GT")
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.bed_motifs(text)
        assert f"at byte {len(_line('rec', 0, 'AC'))} " in L.ribbit_hip_last_error().decode()
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_motifs("rec\t1\t2\tAC\n")      # not a row of 11 columns
    # a text large enough to be cut into parts
    rs = np.random.RandomState(3)
    many = [cc.random_motif(rs, int(k)) for k in rs.randint(1, 40, 150_000)]
    big = "".join(_line("rec", k, m) for k, m in enumerate(many))
    assert len(big) > 2 << 22
    pool, off = ribbit_amd.bed_motifs(big)
    assert pool == "".join(many).encode() and np.array_equal(np.diff(off), [len(m) for m in many])


def test_the_two_texts_byte_for_byte():
    motifs = ["CA", "GATA", "T", "TG", "ACAC", cc.periodic("TCG", 33)]
    name = "rec\twith a tab"
    lines = [_line(name, k, m) for k, m in enumerate(motifs)]
    bed = "".join(lines)
    iv = ribbit_amd.bed_intervals(bed)
    pool, off = ribbit_amd.bed_motifs(bed)
    classes, strands, groups = ribbit_amd.host_record_classes(1000, iv, pool, off)
    want_classes = ["AC", "AGAT", "A", "AC", "ACAC", cc.periodic("ACG", 33)]
    want_strands = ["+", "+", "-", "-", "+", "-"]
    assert unpack(motifs, classes, strands, groups)[:2] == (want_classes, want_strands)
    want = "".join(line[:-1] + f"\t{c}\t{s}\n" for line, c, s in zip(lines, want_classes, want_strands))
    assert ribbit_amd.bed_class_text(bed, classes, off, strands) == want.encode()
    assert ribbit_amd.bed_class_text(bed[:-1], classes, off, strands) == want.encode()      # a last line without its newline
    assert ribbit_amd.bed_class_text("", b"", [0], b"") == b""
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_class_text(bed + "\n", classes, off, strands)                         # one line more than rows
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_class_text(lines[0] + lines[1], b"ACGT", [0, 3, 2], b"++")            # offsets that do not ascend
    # the summary: name, class, length, rows, bases, start and end of the longest row as the BED has them
    summary = f"{name}\tA\t1\t1\t7\t20\t27\n{name}\tAC\t2\t2\t14\t0\t7\n{name}\tACAC\t4\t1\t7\t40\t47\n{name}\tAGAT\t4\t1\t7\t10\t17\n"
    summary += f"{name}\t{cc.periodic('ACG', 33)}\t33\t1\t7\t50\t57\n"
    assert ribbit_amd.class_summary_text(name, iv, classes, off, groups) == summary.encode()
    assert ribbit_amd.class_summary_text(name, iv, classes, off, groups[:0]) == b""
    # start and end are the BED's, not the clipped ones
    far = [(-5, 2000), (990, 3000)]
    c2, s2, g2 = ribbit_amd.host_record_classes(1000, far, ["GT", "AC"])
    assert ribbit_amd.class_summary_text("r", far, c2, [0, 2, 4], g2) == b"r\tAC\t2\t2\t1010\t-5\t2000\n"
    bad = g2.copy()
    bad["longest_row"] = 2
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.class_summary_text("r", far, c2, [0, 2, 4], bad)
    # a text large enough for the writer to work in pieces
    rs = np.random.RandomState(5)
    many = [cc.random_motif(rs, int(k), "AC") for k in rs.randint(1, 9, 200_000)]
    big = [_line("rec", k, m) for k, m in enumerate(many)]
    assert len("".join(big)) > 2 << 22
    pool, off = ribbit_amd.bed_motifs("".join(big))
    classes, strands, _ = ribbit_amd.host_record_classes(10_000_000, ribbit_amd.bed_intervals("".join(big)), pool, off)
    per_row = {u: cc.motif_class(u) for u in set(many)}
    assert ribbit_amd.bed_class_text("".join(big), classes, off, strands) == "".join(
        line[:-1] + "\t%s\t%s\n" % per_row[u] for line, u in zip(big, many)).encode()


# ---- ribbit-hip --class-bed / --motif-summary before the tool touches a GPU: exit status 1 and the exact text on stderr
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_cli_file_names():
    for option in ("--class-bed", "--motif-summary"):
        _dies([option + "="], f"{option} wants a file name")
        _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    _dies(["-i", "in.fa", "--class-bed", "x", "--class-strand", "3"], "unrecognised option '--class-strand'")


@needs_tool
def test_cli_the_two_files_are_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\n")
    for option in ("--class-bed", "--motif-summary"):
        out = tmp_path / "missing" / "out"
        _dies(["-i", tmp_path / "in.fa", option, out], f"{option}: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + ["--class-bed", "--motif-summary"]
    for bad in (6, 7, 8):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]
    # neither needs --overlap-with, and an --overlap-with beside them alone still wants one of its own outputs
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", other, "--class-bed", tmp_path / "x", "--motif-summary", tmp_path / "y"],
          "--overlap-with needs --overlap-bed or --overlap-summary")
    assert not (tmp_path / "x").exists() and not (tmp_path / "y").exists()


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert "\n  --class-bed arg " in r.stderr and "\n  --motif-summary arg " in r.stderr
    assert r.stderr.index("--best-bed arg") < r.stderr.index("--class-bed arg") < r.stderr.index("--motif-summary arg")
    assert "reverse complement" in r.stderr
