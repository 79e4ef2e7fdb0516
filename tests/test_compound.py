"""The rows chained into compound loci without a GPU: ribbit_host_record_compounds against the plain-Python statement of the
contract (tests/compound_contract.py), against a brute force over connected components and against the loci, ribbit_class_labels,
ribbit_compound_text, and ribbit-hip's handling of --compound-bed and --compound-gap up to the point where it would touch a GPU."""
import os
import subprocess

import numpy as np
import pytest

import best_contract
import classes_contract
import compound_contract
import ribbit_amd
from compound_contract import GAPS, I32_MAX, LENGTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
E_ARG = "error -1"


def check_compounds(length, intervals, labels, gap, brute=True):
    compounds, members = ribbit_amd.host_record_compounds(length, intervals, labels, gap)
    assert compounds.dtype == ribbit_amd.COMPOUND_DT and members.dtype == np.int32
    want, want_members = compound_contract.record_compounds(length, intervals, labels, gap)
    assert (compound_contract.as_dicts(compounds), members.tolist()) == (want, want_members), (length, gap)
    compound_contract.check_properties(length, intervals, labels, compounds, members)
    if brute:
        assert compound_contract.against_brute_force(want) == compound_contract.brute_force(length, intervals, labels, gap), (length, gap)
    return compounds, members


def test_the_struct_is_forty_bytes():
    assert ribbit_amd.COMPOUND_DT.itemsize == 40
    assert ribbit_amd.COMPOUND_DT.names == compound_contract.FIELDS


def test_host_twin_on_the_edge_sets():
    for length in LENGTHS:
        for iv, labels in compound_contract.edge_case_sets(length):
            for gap in GAPS:
                check_compounds(length, iv, labels, gap)


def test_reach_decides_not_the_row_before():
    iv, labels = [(10, 200), (20, 30), (240, 260)], [1, 2, 2]
    for gap, chains in ((39, 2), (40, 1), (209, 1)):
        compounds, members = check_compounds(300, iv, labels, gap)
        assert len(compounds) == chains and members.tolist() == [0, 1, 2]
    two, _ = check_compounds(300, iv, labels, 39)
    assert compound_contract.as_dicts(two) == [dict(bases=200, start=10, end=200, rows=2, classes=2, switches=1, overlaps=1, first=0, pad=0),
                                               dict(bases=20, start=240, end=260, rows=1, classes=1, switches=0, overlaps=0, first=2, pad=0)]


def test_host_twin_on_random_records():
    rs = np.random.RandomState(41)
    chains = 0
    for t in range(40):
        length, iv, labels = compound_contract.random_record(rs, t, (1, 3, 50)[t % 3])
        for gap in GAPS:
            chains += len(check_compounds(length, iv, labels, gap, brute=len(iv) <= 200)[0])
    assert chains > 2000


def test_chains_are_the_loci():
    rs = np.random.RandomState(43)
    for t in range(40):
        length, iv, labels = compound_contract.random_record(rs, t, 3)
        chosen, _ = ribbit_amd.host_record_best(length, iv)
        for gap in GAPS:
            compounds, _ = ribbit_amd.host_record_compounds(length, iv, labels, gap)
            loci = ribbit_amd.host_record_loci(length, iv, gap)
            assert all(np.array_equal(compounds[f], loci[f]) for f in ("start", "end", "rows")), (t, gap)
            # rows of which no two overlap: nothing overlaps, and the sum of the widths is what the loci cover
            apart, _ = ribbit_amd.host_record_compounds(length, iv[chosen], labels[chosen], gap)
            loci = ribbit_amd.host_record_loci(length, iv[chosen], gap)
            assert (apart["overlaps"] == 0).all() and np.array_equal(apart["bases"], loci["covered"])
            assert all(np.array_equal(apart[f], loci[f]) for f in ("start", "end", "rows"))


def test_class_labels_against_the_contract():
    rs = np.random.RandomState(47)
    for t in range(30):
        length, iv, motifs = classes_contract.random_record(rs, t)
        classes, _, groups = ribbit_amd.host_record_classes(length, iv, motifs)
        offsets = np.concatenate([[0], np.cumsum([len(m) for m in motifs])])
        labels = ribbit_amd.class_labels(classes, offsets, groups)
        want_classes, _, want_groups = classes_contract.record_classes(length, iv, motifs)
        index = {g[0]: k for k, g in enumerate(want_groups)}
        assert labels.dtype == np.int32 and labels.tolist() == [index[c] for c in want_classes]
    assert ribbit_amd.class_labels(b"", [0], np.zeros(0, ribbit_amd.MOTIF_CLASS_DT)).tolist() == []
    # a row whose class is no group; a group that is no row's
    classes, _, groups = ribbit_amd.host_record_classes(100, [(0, 5), (5, 9), (9, 20)], ["CA", "AG", "AAT"])
    assert ribbit_amd.class_labels(classes, [0, 2, 4, 7], groups).tolist() == [0, 1, 2]
    for fewer in (groups[1:], groups[:1], groups[[0, 2]]):
        with pytest.raises(ribbit_amd.RibbitHipError, match=E_ARG):
            ribbit_amd.class_labels(classes, [0, 2, 4, 7], fewer)
    bad = groups.copy()
    bad["first_row"][1] = 3
    with pytest.raises(ribbit_amd.RibbitHipError, match=E_ARG):
        ribbit_amd.class_labels(classes, [0, 2, 4, 7], bad)
    bad = groups.copy()
    bad["length"][2] = 2
    with pytest.raises(ribbit_amd.RibbitHipError, match=E_ARG):
        ribbit_amd.class_labels(classes, [0, 2, 4, 7], bad)


# ---- the text
ROWS = [(10, 34, "CA", "12", 0), (39, 55, "GA", "8", 1), (100, 120, "AT", "10", 2), (200, 220, "AC", "10", 0), (220, 240, "AC", "10.0", 0),
        (235, 250, "AC", "7.5", 0)]


def _bed(name, rows):
    return "".join(f"{name}\t{s}\t{e}\t{motif}\t1 | {len(motif)}\t{e - s}\t{units}\t0.97\t+\tP\t{e - s}M\n" for s, e, motif, units, _ in rows)


def _text(name, rows, gap, length=1000):
    iv, labels = [(s, e) for s, e, _, _, _ in rows], [label for _, _, _, _, label in rows]
    compounds, members = ribbit_amd.host_record_compounds(length, iv, labels, gap)
    return ribbit_amd.compound_text(name, _bed(name, rows), length, iv, compounds, members).decode()


def test_compound_text_by_hand():
    assert _text("chr1", ROWS, 5) == ("chr1\t10\t55\tc\t2\t2\t40\t(CA)12n5(GA)8\n"
                                      "chr1\t100\t120\tp\t1\t1\t20\t(AT)10\n"
                                      "chr1\t200\t250\ti*\t3\t1\t55\t(AC)10(AC)10.0o5(AC)7.5\n")
    assert _text("chr1", ROWS, 4) == ("chr1\t10\t34\tp\t1\t1\t24\t(CA)12\n"
                                      "chr1\t39\t55\tp\t1\t1\t16\t(GA)8\n"
                                      "chr1\t100\t120\tp\t1\t1\t20\t(AT)10\n"
                                      "chr1\t200\t250\ti*\t3\t1\t55\t(AC)10(AC)10.0o5(AC)7.5\n")
    assert _text("chr1", ROWS[:5], 45) == ("chr1\t10\t120\tc\t3\t3\t60\t(CA)12n5(GA)8n45(AT)10\n"
                                           "chr1\t200\t240\ti\t2\t1\t40\t(AC)10(AC)10.0\n")
    assert _text("chr1", ROWS, I32_MAX) == "chr1\t10\t250\tc*\t6\t3\t115\t(CA)12n5(GA)8n45(AT)10n80(AC)10(AC)10.0o5(AC)7.5\n"
    # the rows in another order: the lines are found by the members' indices; a row clipped by the record's end
    assert _text("chr1", ROWS[::-1], 5) == _text("chr1", ROWS, 5)
    assert _text("chr1", ROWS, 5, length=238).endswith("chr1\t200\t238\ti*\t3\t1\t41\t(AC)10(AC)10.0o3(AC)7.5\n")
    # a name with a tab in it: the columns are found from the right
    assert _text("a\tb", ROWS[:2], 5) == "a\tb\t10\t55\tc\t2\t2\t40\t(CA)12n5(GA)8\n"
    assert _text("", ROWS[2:3], 5) == "\t100\t120\tp\t1\t1\t20\t(AT)10\n"
    assert _text("chr1", [], 5) == ""
    # a last line without its newline counts
    iv, labels = [(s, e) for s, e, _, _, _ in ROWS], [row[4] for row in ROWS]
    compounds, members = ribbit_amd.host_record_compounds(1000, iv, labels, 5)
    assert ribbit_amd.compound_text("chr1", _bed("chr1", ROWS)[:-1], 1000, iv, compounds, members).decode() == _text("chr1", ROWS, 5)


def test_compound_text_refuses_what_does_not_fit():
    iv, labels = [(s, e) for s, e, _, _, _ in ROWS], [row[4] for row in ROWS]
    bed = _bed("chr1", ROWS)
    compounds, members = ribbit_amd.host_record_compounds(1000, iv, labels, 5)

    def refused(bed=bed, iv=iv, compounds=compounds, members=members, length=1000):
        with pytest.raises(ribbit_amd.RibbitHipError, match=E_ARG):
            ribbit_amd.compound_text("chr1", bed, length, iv, compounds, members)

    refused(bed="".join(bed.splitlines(keepends=True)[:5]))                  # a member that is no line of the BED text
    refused(members=[0, 1, 2, 3, 4, 6])
    refused(members=[0, 1, 2, 3, 4, -1])
    refused(iv=iv[:5])                                                       # ... or no row
    refused(members=members[:5])                                             # first / rows outside members
    for field, value in (("first", -1), ("first", 6), ("rows", 0), ("rows", -2), ("rows", 4), ("rows", I32_MAX), ("first", I32_MAX)):
        bad = compounds.copy()
        bad[field][2] = value
        refused(compounds=bad)
    refused(bed=bed.replace("\t0.97\t+", "\t0.97+"))                         # a line that is not a row
    refused(bed="chr1\n" * 6)
    refused(length=230)                                                      # a member that is empty in a record that short
    refused(length=-1)
    refused(length=1 << 31)
    assert ribbit_amd.compound_text("chr1", bed, 1000, iv, compounds, members).decode() == _text("chr1", ROWS, 5)


def test_bad_arguments_of_the_host_twin():
    for gap in (-1, -(1 << 31)):
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"{E_ARG}: gap {gap} is negative"):
            ribbit_amd.host_record_compounds(100, [(0, 5)], [0], gap)
    for length in (-1, 1 << 31):
        with pytest.raises(ribbit_amd.RibbitHipError, match=E_ARG):
            ribbit_amd.host_record_compounds(length, [(0, 5)], [0], 0)
    with pytest.raises(ValueError):
        ribbit_amd.host_record_compounds(100, [(0, 5)], [0, 1], 0)
    with pytest.raises(ValueError):
        ribbit_amd.host_record_compounds(100, [(0, 5)], [1 << 31], 0)
    with pytest.raises(ValueError):
        ribbit_amd.host_record_compounds(100, [(0, 5)], [0], 1 << 31)
    assert [len(x) for x in ribbit_amd.host_record_compounds(0, [(0, 5), (-3, 9)], [1, 2], 0)] == [0, 0]
    assert [len(x) for x in ribbit_amd.host_record_compounds(100, [], [], 0)] == [0, 0]
    assert [len(x) for x in ribbit_amd.host_record_compounds(100, [(9, 5), (100, 200)], [1, 2])] == [0, 0]


# ---- the tool's arguments
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (args, r.returncode, r.stderr)
    assert r.stdout == "" and r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_compound_gap_needs_compound_bed():
    _dies(["--compound-gap", "5"], "--compound-gap needs --compound-bed")
    _dies(["-i", "in.fa", "--compound-gap=5"], "--compound-gap needs --compound-bed")
    _dies(["--compound-gap", "5", "--loci-bed", "out", "--best-bed", "out2"], "--compound-gap needs --compound-bed")
    # of two orphans the first in the order of the outputs is reported
    _dies(["--compound-gap", "5", "--loci-gap", "1"], "--loci-gap needs --loci-bed")


@needs_tool
@pytest.mark.parametrize("value", ["-1", "x", "", "2147483648", "12345678901", "1.5", "0x10"])
def test_rejected_compound_gaps(value):
    message = f"--compound-gap wants a whole number of bases (0 .. 2147483647), got '{value}'"
    _dies(["--compound-gap", value], message)
    _dies(["-i", "in.fa", "--compound-bed", "out", f"--compound-gap={value}"], message)


@needs_tool
def test_file_name_and_missing_argument(tmp_path):
    _dies(["--compound-bed="], "--compound-bed wants a file name")
    _dies(["-i", "in.fa", "--compound-bed", ""], "--compound-bed wants a file name")
    for option in ("--compound-bed", "--compound-gap"):
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    out = tmp_path / "missing" / "out"
    for gap in ("0", "100", "2147483647"):      # the limits parse and the tool goes on to open its files, this one last
        _dies(["-i", tmp_path / "in.fa", "--compound-gap", gap, "--compound-bed", out], f"--compound-bed: cannot open '{out}' for writing")
    best = tmp_path / "best.bed"
    _dies(["-i", tmp_path / "in.fa", "--compound-bed", out, "--best-bed", best], f"--compound-bed: cannot open '{out}' for writing")
    assert best.read_bytes() == b"" and not (tmp_path / "missing").exists()


@needs_tool
def test_help_names_both_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    for option in ("--compound-bed", "--compound-gap"):
        assert f"\n  {option} arg " in r.stderr, option
    assert "Default: 100\n" in r.stderr.split("--compound-gap arg")[1]
