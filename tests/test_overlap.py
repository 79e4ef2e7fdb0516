"""The rows' overlap with a second set of intervals without a GPU: ribbit_host_record_overlap and ribbit_bed_overlap_text
against the numpy statement of the contract (tests/overlap_contract.py), the argument errors, and simulate.truth_bed_text."""
import ctypes as C
import os

import numpy as np
import pytest

import overlap_contract
import ribbit_amd
from ribbit_amd.simulate import simulate_sequence, truth_bed_text

I32_MAX = (1 << 31) - 1
LENGTHS = (0, 1, 31, 32, 33, 255, 256, 257, 16383, 16384, 16385)


def check(length, rows, other):
    per_row, totals = ribbit_amd.host_record_overlap(length, rows, other)
    assert per_row.dtype == np.int32 and per_row.shape == (len(rows), 2)
    want_rows, want_totals = overlap_contract.record_overlap(length, rows, other)
    assert per_row.tolist() == want_rows, length
    assert totals == want_totals, length
    return per_row, totals


@pytest.mark.parametrize("length", LENGTHS)
def test_edge_case_sets(length):
    for what, rows, other in overlap_contract.edge_case_sets(length):
        per_row, totals = check(length, rows, other)
        # the two sets change places: the totals do too
        _, swapped = check(length, other, rows)
        assert [swapped[k] for k in ("other", "other_hit", "rows", "rows_hit", "other_bases", "rows_bases", "both_bases")] == \
               [totals[k] for k in overlap_contract.TOTALS], what
        assert totals["both_bases"] <= min(totals["rows_bases"], totals["other_bases"]) <= length


def test_what_the_shapes_say():
    per_row, totals = check(300, [(10, 20), (40, 50), (64, 96)], [(20, 40), (0, 10), (50, 64), (96, 97), (32, 64)])
    assert per_row.tolist() == [[0, 0], [1, 10], [0, 0]]                 # abutting on either side is no overlap
    assert (totals["rows_hit"], totals["other_hit"], totals["both_bases"]) == (1, 1, 10)
    per_row, totals = check(300, [(20, 30)] * 3, [(25, 28)] * 4 + [(0, 0)])
    assert per_row.tolist() == [[4, 3]] * 3                              # duplicates each count, the bases of their union once
    assert totals == dict(rows=3, rows_hit=3, other=4, other_hit=4, rows_bases=10, other_bases=3, both_bases=3)
    per_row, totals = check(100, [(50, 10), (-5, 3), (99, 500)], [(-(1 << 31), I32_MAX)])
    assert per_row.tolist() == [[0, 0], [1, 3], [1, 1]]
    assert totals == dict(rows=2, rows_hit=2, other=1, other_hit=1, rows_bases=4, other_bases=100, both_bases=4)
    _, totals = check(100, [(1, 5)], [])
    assert totals == dict(rows=1, rows_hit=0, other=0, other_hit=0, rows_bases=4, other_bases=0, both_bases=0)


def test_random_sets():
    rs = np.random.RandomState(2026)
    for t in range(200):
        length = int(rs.choice([1, 31, 33, 257, 1000, rs.randint(0, 5000)]))
        rows, other = overlap_contract.random_sets(length, rs, int(rs.randint(0, 40)), int(rs.randint(0, 40)), 30 if t % 2 else 900)
        check(length, rows, other)


def test_overlap_text():
    name = "chr\tX"                       # (a name with a tab in it: nothing is parsed, the line is kept byte for byte)
    bed = "".join(f"{name}\t{s}\t{s + 9}\tAC\t2 | 2\t9\t4\t0.9\t+\tSEED-5\t9=\n" for s in (5, 50, 7))
    per_row = [(0, 0), (3, 9), (2147483647, 1)]
    text = ribbit_amd.bed_overlap_text(bed, per_row).decode()
    assert text == overlap_contract.overlap_lines(bed, per_row)
    lines = text.splitlines()
    assert [l.split("\t")[-2:] for l in lines] == [["0", "0"], ["3", "9"], ["2147483647", "1"]]
    assert all(len(l.split("\t")) == 14 for l in lines)                   # 13 columns and the name's own tab
    assert "".join(l.rsplit("\t", 2)[0] + "\n" for l in lines) == bed
    # a last row without its newline is still a row
    assert ribbit_amd.bed_overlap_text(bed[:-1], per_row).decode() == text
    assert ribbit_amd.bed_overlap_text("", []) == b""
    for wrong in (per_row[:2], per_row + [(1, 1)], []):
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            ribbit_amd.bed_overlap_text(bed, wrong)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_overlap_text("", per_row)


def test_overlap_text_of_many_rows():
    """megabytes of rows: the line starts are found and the lines written in pieces on several threads"""
    rs = np.random.RandomState(8)
    n = 120_000
    lines = [f"chr\t{s}\t{s + 30}\tACG\t3 | 3\t30\t10\t0.9\t+\tSEED-5\t{'10=' * (1 + s % 9)}\n" for s in rs.randint(0, 1 << 30, n)]
    bed = "".join(lines)
    assert len(bed) > 5 << 20
    per_row = rs.randint(0, 1 << 20, (n, 2))
    text = ribbit_amd.bed_overlap_text(bed, per_row).decode().splitlines(keepends=True)
    assert len(text) == n
    for k in list(range(0, n, 997)) + [n - 1]:
        assert text[k] == f"{lines[k][:-1]}\t{per_row[k][0]}\t{per_row[k][1]}\n"


def test_bad_arguments_rejected(hip_lib):
    L = hip_lib
    per_row, text, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    totals = ribbit_amd.OverlapTotals()
    iv = (C.c_int32 * 2)(0, 3)
    too_many = (1 << 31)
    assert L.ribbit_host_record_overlap(10, None, 1, iv, 1, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(10, iv, 1, None, 1, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(10, iv, 1, iv, 1, None, C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(10, iv, 1, iv, 1, C.byref(per_row), None) == -1
    assert L.ribbit_host_record_overlap(10, iv, too_many, iv, 1, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(10, iv, 1, iv, too_many, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(-1, iv, 1, iv, 1, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(1 << 31, iv, 1, iv, 1, C.byref(per_row), C.byref(totals)) == -1
    assert L.ribbit_host_record_overlap(10, None, 0, None, 0, C.byref(per_row), C.byref(totals)) == 0 and totals.as_dict() == dict.fromkeys(overlap_contract.TOTALS, 0)
    L.ribbit_intervals_free(per_row)
    # a null handle is refused before anything else (no GPU needed to say so)
    assert L.ribbit_hip_record_overlap(None, iv, 1, iv, 1, C.byref(per_row), C.byref(totals)) == -1
    assert b"null handle" in L.ribbit_hip_last_error()
    assert L.ribbit_bed_overlap_text(None, 5, None, 0, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_overlap_text(b"a\n", 2, None, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_overlap_text(b"", 0, None, 0, None, C.byref(n)) == -1
    assert L.ribbit_bed_overlap_text(b"", 0, None, 0, C.byref(text), None) == -1
    assert ribbit_amd.OVERLAP_TOTALS == overlap_contract.TOTALS


def test_truth_bed_text():
    seq, truth = simulate_sequence(30_000, 5, 2, 30)
    text = truth_bed_text("rec 1", truth)
    assert text.endswith("\n") and len(text.splitlines()) == len(truth) > 5
    for line, (start, end, m, motif) in zip(text.splitlines(), truth):
        assert line == f"rec 1\t{start}\t{end}\t{m}\t{motif}" and len(motif) == m and 0 <= start < end <= len(seq)
    assert truth_bed_text("x", []) == ""
    # the truth against itself: everything is found, base for base
    pairs = [t[:2] for t in truth]
    per_row, totals = ribbit_amd.host_record_overlap(len(seq), pairs, pairs)
    assert totals["rows_hit"] == totals["other_hit"] == len(truth) and totals["both_bases"] == totals["rows_bases"] == sum(e - s for s, e in pairs)
    assert per_row.tolist() == [[1, e - s] for s, e in pairs]


def test_new_files_are_part_of_every_build():
    """overlap.hip and api_overlap.cpp are in the Makefile's NAMES: the sanitizer builds instrument the new host code too"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [l for l in open(os.path.join(root, "ribbit_amd", "csrc", "Makefile")) if l.startswith("NAMES")][0].split()
    assert "overlap" in names and "api_overlap" in names
