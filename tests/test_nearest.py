"""The nearest target of every query without a GPU: ribbit_host_record_nearest against the plain-Python statement of the
contract (tests/nearest_contract.py), what follows from the contract, the two text functions byte for byte against the plain
formatter, every refusal with its text, and ribbit-hip's handling of --nearest-bed and --nearest-other-bed up to the point where
it would touch a GPU."""
import os
import subprocess

import numpy as np
import pytest

import nearest_contract as nc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
LENGTHS = (0, 1, 64, 1000)
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed"]
NEW_OUTPUTS = ["--nearest-bed", "--nearest-other-bed"]


def check(length, queries, targets, what=None):
    got = nc.as_tuples(ribbit_amd.host_record_nearest(length, queries, targets))
    want = nc.record_nearest(length, queries, targets)
    assert got == want, (length, what)
    nc.check_properties(length, queries, targets, want)
    assert nc.record_nearest_without_loops(length, queries, targets).tolist() == [list(r) for r in want], (length, what)
    return want


@pytest.mark.parametrize("length", LENGTHS)
def test_host_twin_on_the_edge_sets(length):
    for what, queries, targets in nc.edge_case_sets(length):
        forward = check(length, queries, targets, what)
        backward = check(length, targets, queries, what)
        nc.check_symmetry(length, queries, targets, forward, backward)
        nc.check_symmetry(length, targets, queries, backward, forward)


def test_the_shapes_by_hand():
    """the words of the contract on a record of 100 bases: the furthest-reaching container, the first overlapping target, both
    neighbours whatever the kind, an abutting target at distance 0"""
    targets = [(10, 40), (10, 50), (5, 50), (45, 60), (70, 80), (60, 70), (0, 5)]
    got = nc.as_tuples(ribbit_amd.host_record_nearest(100, [(12, 20), (42, 65), (62, 63), (85, 90), (0, 5), (5, 10), (100, 120)], targets))
    assert got == [
        (nc.INSIDE, 2, 6, 7, 3, 25),        # three containers: 5..50 and 10..50 reach furthest, 5..50 starts first
        (nc.OVER, 2, 0, 2, 4, 5),           # 5..50, 10..50, 45..60 and 60..70 overlap: 5..50 is the first by start
        (nc.INSIDE, 5, 3, 2, 4, 7),
        (nc.APART, -1, 4, 5, -1, -1),
        (nc.INSIDE, 6, -1, -1, 2, 0),       # 5..50 abuts on the right
        (nc.INSIDE, 2, 6, 0, 0, 0),         # inside 5..50 and still between 0..5 and 10..40, abutting both; of 10..40 and 10..50 the shorter comes first
        nc.NOTHING,                         # clipped away
    ]


@pytest.mark.parametrize("length", LENGTHS)
def test_random_sets(length):
    rs = np.random.RandomState(1000 + length)
    for n_targets in (0, 1, 2, 3, 300):
        for longest in (4, 60):
            queries, targets = nc.random_sets(length, rs, 120, n_targets, longest)
            forward = check(length, queries, targets, (n_targets, longest))
            backward = nc.record_nearest(length, targets, queries)
            nc.check_symmetry(length, queries, targets, forward, backward)


def test_bad_arguments():
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1.*a record of -1 bases"):
        ribbit_amd.host_record_nearest(-1, [(0, 1)], [(0, 1)])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1.*a record of 2147483648 bases"):
        ribbit_amd.host_record_nearest(1 << 31, [(0, 1)], [(0, 1)])
    L = ribbit_amd.load_library()
    assert L.ribbit_host_record_nearest(10, None, 1, None, 0, None) == -1 and b"null argument" in L.ribbit_hip_last_error()
    L.ribbit_nearest_free(None)


# ---- the two texts
def _line(name, s, e, motif):
    return f"{name}\t{s}\t{e}\t{motif}\t.\t.\t{(e - s) // len(motif)}\t.\t.\t.\t{e - s}=\n"


ROWS = [(3, 15), (20, 32), (40, 52), (60, 90), (95, 99), (-4, 0)]
MOTIFS = ["AC", "ACG", "A", "ACGT", "TG", "C"]
TARGETS = [(0, 35), (38, 45), (70, 80), (2147483647, -2147483648), (-7, 1000), (33, 38)]
LABELS = ["gene one", ".", "exon 2;x", "reversed", "all", "2"]


def _bed(name="rec"):
    return "".join(_line(name, s, e, m) for (s, e), m in zip(ROWS, MOTIFS))


def test_the_two_texts_byte_for_byte():
    length = 100
    near = ribbit_amd.host_record_nearest(length, ROWS, TARGETS)
    bed = _bed()
    want = nc.nearest_lines(bed, nc.as_tuples(near), TARGETS, LABELS)
    assert ribbit_amd.bed_nearest_text(bed, near, TARGETS, LABELS) == want.encode()
    assert want.splitlines()[0] == bed.splitlines()[0] + "\tin\tall\t-7\t1000\t.\t.\t2\t18"
    assert all(len(l.split("\t")) == 19 for l in want.splitlines())
    # a last line without its newline is written with one; a name with a tab in it and a label with blanks stay as they are
    assert ribbit_amd.bed_nearest_text(bed[:-1], near, TARGETS, LABELS) == want.encode()
    tabbed = _bed("a\tb c")
    assert ribbit_amd.bed_nearest_text(tabbed, near, TARGETS, LABELS) == nc.nearest_lines(tabbed, nc.as_tuples(near), TARGETS, LABELS).encode()
    # no targets at all: '.' throughout
    none = ribbit_amd.host_record_nearest(length, ROWS, [])
    assert ribbit_amd.bed_nearest_text(bed, none, [], []) == "".join(l + "\t.\t.\t.\t.\t.\t.\t.\t.\n" for l in bed.splitlines()).encode()
    assert ribbit_amd.bed_nearest_text("", [], TARGETS, LABELS) == b""
    # the other direction: the rows are the targets, their motifs the labels, start and end as the BED has them
    back = ribbit_amd.host_record_nearest(length, TARGETS, ROWS)
    want = nc.other_lines("rec", TARGETS, LABELS, nc.as_tuples(back), ROWS, MOTIFS)
    assert ribbit_amd.nearest_other_text("rec", TARGETS, LABELS, back, ROWS, MOTIFS) == want.encode()
    assert want.splitlines()[1] == "rec\t38\t45\t.\tover\tA\t40\t52\tACG\t6\tACGT\t15"
    assert want.splitlines()[3] == "rec\t2147483647\t-2147483648\treversed" + "\t." * 8
    assert all(len(l.split("\t")) == 12 for l in want.splitlines())
    assert ribbit_amd.nearest_other_text("rec", [], [], [], ROWS, MOTIFS) == b""
    # pools with offsets, as the command-line tool and ribbit_bed_motifs hand them over
    pool, off = ribbit_amd.bed_motifs(bed)
    label_pool = "".join(LABELS)
    label_off = np.concatenate([[0], np.cumsum([len(l) for l in LABELS])])
    assert ribbit_amd.nearest_other_text("rec", TARGETS, label_pool, back, ROWS, pool, label_off, off) == want.encode()


def test_every_refusal_of_the_texts():
    near = ribbit_amd.host_record_nearest(100, ROWS, TARGETS)
    back = ribbit_amd.host_record_nearest(100, TARGETS, ROWS)
    bed = _bed()
    label_pool = "".join(LABELS)
    label_off = np.concatenate([[0], np.cumsum([len(l) for l in LABELS])])

    def refused(message, call):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1") as err:
            call()
        assert message in str(err.value), str(err.value)

    def with_field(array, i, field, value):
        changed = array.copy()
        changed[field][i] = value
        return changed

    refused("the BED text has 5 lines, not the 6 of the rows", lambda: ribbit_amd.bed_nearest_text("".join(bed.splitlines(True)[:5]), near, TARGETS, LABELS))
    refused("the BED text has 6 lines, not the 5 of the rows", lambda: ribbit_amd.bed_nearest_text(bed, near[:5], TARGETS, LABELS))
    for kind in (-1, 3):
        refused(f"row 2: a kind of {kind}, not 0, 1 or 2", lambda: ribbit_amd.bed_nearest_text(bed, with_field(near, 2, "kind", kind), TARGETS, LABELS))
        refused(f"interval 4: a kind of {kind}, not 0, 1 or 2", lambda: ribbit_amd.nearest_other_text("rec", TARGETS, LABELS, with_field(back, 4, "kind", kind), ROWS, MOTIFS))
    for field, words in (("hit", "hit"), ("left", "left neighbour"), ("right", "right neighbour")):
        for value in (-2, 6, 2147483647):
            refused(f"row 1: its {words} {value} is none of the 6 intervals", lambda: ribbit_amd.bed_nearest_text(bed, with_field(near, 1, field, value), TARGETS, LABELS))
            refused(f"interval 5: its {words} {value} is none of the 6 rows",
                    lambda: ribbit_amd.nearest_other_text("rec", TARGETS, LABELS, with_field(back, 5, field, value), ROWS, MOTIFS))
    # (the last valid index is taken)
    assert ribbit_amd.bed_nearest_text(bed, with_field(near, 1, "hit", 5), TARGETS, LABELS).splitlines()[1].split(b"\t")[12:14] == [b"2", b"33"]
    # label offsets that are negative, do not ascend or leave the pool
    down = label_off.copy()
    down[3] = down[2] - 1
    beyond = label_off.copy()
    beyond[-1] += 1
    below = label_off.copy()
    below[0] = -1
    for off, message in ((down, "interval 2: the labels' offsets do not ascend"), (beyond, f"the labels' offsets end at {len(label_pool) + 1}, behind the {len(label_pool)} bytes of their pool"),
                         (below, "the labels' offsets start at -1, below 0")):
        refused(message, lambda: ribbit_amd.bed_nearest_text(bed, near, TARGETS, label_pool, off))
        refused(message, lambda: ribbit_amd.nearest_other_text("rec", TARGETS, label_pool, back, ROWS, MOTIFS, off))
    pool, off = ribbit_amd.bed_motifs(bed)
    down = off.copy()
    down[1] = 9
    beyond = off.copy()
    beyond[-1] += 2
    refused("row 1: the motifs' offsets do not ascend", lambda: ribbit_amd.nearest_other_text("rec", TARGETS, LABELS, back, ROWS, pool, None, down))
    refused("the motifs' offsets end at", lambda: ribbit_amd.nearest_other_text("rec", TARGETS, LABELS, back, ROWS, pool, None, beyond))
    # a NUL inside the pool ends it
    refused("behind the 4 bytes of their pool", lambda: ribbit_amd.bed_nearest_text(bed, near, TARGETS, label_pool[:4] + "\0" + label_pool[5:], label_off))
    L = ribbit_amd.load_library()
    assert L.ribbit_bed_nearest_text(None, 0, None, 0, None, None, None, 0, None, None) == -1 and b"null argument" in L.ribbit_hip_last_error()


def test_texts_written_in_pieces():
    """a BED text large enough for the writer to work in pieces (4 MB each), from the twin's result"""
    rs = np.random.RandomState(8)
    n = 120_000
    starts = np.sort(rs.randint(0, 3_000_000, n))
    rows = np.stack([starts, starts + rs.randint(1, 60, n)], 1)
    bed = "".join(f"chr\t{s}\t{e}\tACGTAC\t.\t.\t{(e - s) // 6}\t.\t.\t.\t{'0000000001=' * 4}{e - s}=\n" for s, e in rows.tolist())
    assert len(bed) > 2 << 22
    t_starts = rs.randint(-5, 3_000_100, 4_000)
    targets = np.stack([t_starts, t_starts + rs.randint(-3, 900, 4_000)], 1)
    labels = [f"t{j}" for j in range(len(targets))]
    near = ribbit_amd.host_record_nearest(3_000_050, rows, targets)
    assert ribbit_amd.bed_nearest_text(bed, near, targets, labels) == nc.nearest_lines(bed, nc.as_tuples(near), targets.tolist(), labels).encode()
    back = ribbit_amd.host_record_nearest(3_000_050, targets, rows)
    motifs = ["ACGTAC"] * n
    assert ribbit_amd.nearest_other_text("chr", targets, labels, back, rows, motifs) == nc.other_lines("chr", targets.tolist(), labels, nc.as_tuples(back), rows.tolist(),
                                                                                                      motifs).encode()


# ---- ribbit-hip --nearest-bed / --nearest-other-bed before the tool touches a GPU: exit status 1 and the exact text on stderr
def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == ""
    assert r.stderr == message, args


def _dies(args, message):
    _fails(args, "ribbit-hip: " + message + "\n")


@pytest.fixture
def other(tmp_path):
    path = tmp_path / "other.bed"
    path.write_text("a\t1\t5\tgene\n")
    return path


@needs_tool
def test_cli_the_options_need_each_other(other, tmp_path):
    for option in NEW_OUTPUTS:
        _dies([option, "out"], f"{option} needs --overlap-with")
        _dies(["-i", "in.fa", f"{option}=out"], f"{option} needs --overlap-with")
        # --overlap-with with a nearest output alone is accepted: the next complaint is the missing input
        _fails(["--overlap-with", other, option, tmp_path / "missing" / "out"], "ERROR: Please specify an input fasta file!\n")
    # without their input: the first in the order of the fourteen
    _dies(["--nearest-other-bed", "o", "--nearest-bed", "b"], "--nearest-bed needs --overlap-with")
    _dies(["--nearest-bed", "b", "--overlap-summary", "s"], "--overlap-summary needs --overlap-with")
    _dies(["--nearest-other-bed", "o", "--purity-bed", "p"], "--nearest-other-bed needs --overlap-with")
    # --overlap-with with none of the four outputs that need it: the message as it was
    _dies(["--overlap-with", other], "--overlap-with needs --overlap-bed or --overlap-summary")
    _dies(["-i", "in.fa", "--overlap-with", other, "--purity-bed", "p"], "--overlap-with needs --overlap-bed or --overlap-summary")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_file_names():
    for option in NEW_OUTPUTS:
        _dies([option + "="], f"{option} wants a file name")
        _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    _dies(["-i", "in.fa", "--nearest-bed", "x", "--nearest-gap", "3"], "unrecognised option '--nearest-gap'")


@needs_tool
def test_cli_the_two_files_are_opened_last(tmp_path, other):
    for option in NEW_OUTPUTS:
        out = tmp_path / "missing" / "out"
        _dies(["-i", tmp_path / "in.fa", "--overlap-with", other, option, out], f"{option}: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + NEW_OUTPUTS
    for bad in (11, 12, 13):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]


@needs_tool
def test_cli_other_files_with_and_without_labels(tmp_path):
    """what the reader takes has not changed: lines of three columns, an empty fourth column, a fourth column with blanks, further
    columns, no final newline -- the run then ends at the first output file that cannot be made; and what it refuses is refused
    in the same words beside the new outputs"""
    out = tmp_path / "missing" / "out"
    for text in ("a\t1\t5\n", "a\t1\t5\t\n", "a\t1\t5\t\t7\n", "a\t1\t5\tgene one\t0\t+\nb c\t9\t2\nb c\t-5\t-1\texon", "# only a comment\n", ""):
        bed = tmp_path / "other.bed"
        bed.write_text(text)
        for option in NEW_OUTPUTS:
            _dies(["-i", tmp_path / "in.fa", "--overlap-with", bed, option, out], f"{option}: cannot open '{out}' for writing")
    bed.write_text("a\t1\t5\tgene\nb\t7\n")
    _dies(["-i", tmp_path / "in.fa", "--overlap-with", bed, "--nearest-bed", tmp_path / "n.bed"], f"--overlap-with: line 2 of '{bed}' is not a BED line (name, start, end)")
    assert not (tmp_path / "n.bed").exists()


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    assert "\n  --nearest-bed arg " in r.stderr and "\n  --nearest-other-bed arg " in r.stderr
    assert r.stderr.index("--purity-bed arg") < r.stderr.index("--nearest-bed arg") < r.stderr.index("--nearest-other-bed arg")
    assert "bedtools\n" in r.stderr and "closest" in r.stderr
    at = r.stderr.index("\n  --overlap-with arg ")
    assert "column 4" in r.stderr[at:r.stderr.index("\n  --overlap-bed arg ")]
