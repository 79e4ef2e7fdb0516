"""Merged loci and the density track without a GPU: ribbit_host_record_loci, ribbit_host_record_density and
ribbit_bed_loci_text against the numpy statement of the contract (tests/loci_contract.py), and the command-line
options' refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loci_contract
import ribbit_amd
from cases import simulated_cases
from mask_contract import masked_body
from oracle_lib import Oracle

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 300, 1000)
GAPS = (0, 1, 5, 1000, I32_MAX)


def windows_for(length):
    return sorted({w for w in (1, 2, 31, 32, 33, 64, 1000, length - 1, length, length + 1, I32_MAX) if w >= 1})


def check_loci(length, intervals, gap=0):
    got = ribbit_amd.host_record_loci(length, intervals, gap)
    assert got.dtype == ribbit_amd.LOCUS_DT
    want = loci_contract.record_loci(length, intervals, gap)
    assert got.tolist() == want, (length, gap)
    return want


def check_density(length, intervals, window):
    got = ribbit_amd.host_record_density(length, intervals, window)
    assert got.dtype == np.int32
    want = loci_contract.record_density(length, intervals, window)
    assert got.tolist() == want, (length, window)
    return want


def check_all(length, intervals, gaps=(0, 5), windows=None):
    for gap in gaps:
        check_loci(length, intervals, gap)
    for w in windows_for(length) if windows is None else windows:
        check_density(length, intervals, w)


def non_empty_rows(length, intervals):
    iv = np.asarray(intervals, np.int64).reshape(-1, 2)
    return int((np.maximum(iv[:, 0], 0) < np.minimum(iv[:, 1], length)).sum())


def check_invariants(length, intervals, gap, window):
    loci = check_loci(length, intervals, gap)
    density = check_density(length, intervals, window)
    masked = masked_body(b"A" * length, intervals, "hard", 0).count(b"N")
    assert sum(l[3] for l in loci) == sum(density) == masked
    assert sum(l[2] for l in loci) == non_empty_rows(length, intervals)
    for a, b in zip(loci, loci[1:]):
        assert a[0] < a[1] and b[0] - a[1] >= gap + 1
    for l in loci:
        assert 0 <= l[0] < l[1] <= length and l[2] >= 1 and 1 <= l[3] <= l[1] - l[0]
        if gap == 0:
            assert l[3] == l[1] - l[0]


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_and_windows(length):
    for iv in ([], [(0, 1)], [(0, length)], [(3, 9), (5, 20)], [(-5, 4), (length - 2, length + 50)], [(I32_MIN, I32_MAX)],
               [(length - 1, length)], [(length, length + 1)], [(-1, 0)]):
        check_all(length, iv)
    assert ribbit_amd.host_record_loci(length, []).shape == (0,)
    assert ribbit_amd.host_record_density(length, [], 7).tolist() == [0] * -(-length // 7)
    if length:
        assert ribbit_amd.host_record_loci(length, [(I32_MIN, I32_MAX)]).tolist() == [(0, length, 1, length, 0)]


def test_row_shapes():
    length = 300
    plain = [(10, 50), (200, 220)]
    cases = {
        "overlapping": [(10, 50), (40, 90), (45, 46), (10, 50)],
        "unsorted": [(200, 220), (5, 9), (100, 101), (60, 70)],
        "out of range": [(-100, -1), (300, 400), (-7, 3), (299, 1000), (I32_MIN, I32_MAX)],
        "duplicates": [(20, 30)] * 5 + [(100, 130)] * 3,
        "nested stack": [(10, 200), (20, 190), (30, 180), (40, 170), (50, 60), (10, 200)],
        "abutting": [(10, 20), (20, 30), (30, 31), (40, 50)],
        "whole record": [(0, 300)],
    }
    for iv in cases.values():
        check_all(length, iv, gaps=GAPS)
    assert [l[:3] for l in check_loci(length, cases["abutting"])] == [(10, 31, 3), (40, 50, 1)]
    assert check_loci(length, cases["nested stack"]) == [(10, 200, 6, 190, 0)]
    # reversed and zero-length rows: the same result as without them (their indices shifted), and best_row never names one
    useless = [(50, 10), (20, 20), (90, -5), (400, 500), (-9, 0)]
    want = check_loci(length, plain)
    mixed = [useless[0], plain[0], useless[1], useless[2], plain[1], useless[3], useless[4]]
    got = check_loci(length, mixed)
    assert [l[:4] for l in got] == [l[:4] for l in want] and [l[4] for l in got] == [1, 4]
    assert check_loci(length, useless) == []
    for w in windows_for(length):
        assert check_density(length, mixed, w) == check_density(length, plain, w)
        assert sum(check_density(length, useless, w)) == 0


def test_bitmap_word_boundaries():
    length = 32 * 9 + 5
    for k in (1, 2, 4, 8):
        for s in (32 * k - 1, 32 * k, 32 * k + 1):
            for e in (s + 1, 32 * k + 31, 32 * k + 32, 32 * k + 33, 32 * (k + 1) - 1):
                check_all(length, [(s, e)], windows=(1, 31, 32, 33, 64))
                check_all(length, [(0, s), (e, length)], windows=(1, 31, 32, 33, 64))
                check_all(length, [(s, e), (e, e + 1), (s - 40, s - 1)], gaps=(0, 1), windows=(32,))


@pytest.mark.parametrize("gap", GAPS)
def test_gaps_exactly_at_the_limit(gap):
    length = 5000 if gap <= 1000 else 300
    d = min(gap, 1000 if gap <= 1000 else 100)
    rows = [(10, 20), (20 + d, 40 + d), (41 + d + d, 60 + d + d), (4990, 4999)]
    loci = check_loci(length, rows, gap)
    if gap <= 1000:      # gaps of exactly gap (joined) and gap + 1 (not joined)
        assert [l[:4] for l in loci][:2] == [(10, 40 + gap, 2, 30), (41 + 2 * gap, 60 + 2 * gap, 1, 19)]
    else:
        assert len(loci) == 1 and loci[0][2] == 3
    for g in {max(gap - 1, 0), gap, min(gap + 1, I32_MAX)}:
        check_invariants(length, rows, g, 64)


def test_ties_go_to_the_lowest_index():
    length = 400
    rows = [(100, 130), (90, 120), (110, 140), (95, 100), (300, 310), (301, 311), (299, 309), (302, 303)]
    loci = check_loci(length, rows)
    assert [l[4] for l in loci] == [0, 4]
    rs = np.random.RandomState(3)
    for _ in range(30):
        perm = rs.permutation(len(rows))
        got = check_loci(length, [rows[i] for i in perm])
        longest = [min(j for j, i in enumerate(perm) if i in block and rows[i][1] - rows[i][0] == 30 - 20 * (block[0] > 3))
                   for block in ((0, 1, 2, 3), (4, 5, 6, 7))]
        assert [l[4] for l in got] == longest
    # clipping decides the length that counts
    assert check_loci(100, [(90, 200), (80, 95), (-50, 12), (0, 13)])[0][4] == 3


def test_random_row_sets():
    rs = np.random.RandomState(2025)
    for t in range(300):
        length = int(rs.choice([1, 31, 33, 200, 1000, rs.randint(0, 5000)]))
        n = rs.randint(0, 40)
        iv = np.stack([rs.randint(-50, length + 50, n), rs.randint(-50, length + 50, n)], 1) if n else np.zeros((0, 2), int)
        if n and rs.rand() < 0.5:         # short rows, so that gaps stay
            iv[:, 1] = iv[:, 0] + rs.randint(-3, 30, n)
        gap = int(rs.choice(GAPS + (2, 17)))
        window = int(rs.choice(windows_for(length) + [7, 100]))
        check_invariants(length, iv, gap, window)


def _oracle_bed(name):
    seq = simulated_cases()[0][1][:40_000]
    with Oracle(seq, 2, 30) as o:
        o.run_all()
        return seq, o.refine_bed(name)


def test_loci_text_of_oracle_rows():
    name = "chr\tX"                     # (a name with a tab in it: the row's columns are found from the right)
    seq, bed = _oracle_bed(name)
    rows = ribbit_amd.bed_intervals(bed)
    assert len(rows) > 100
    for gap, window in ((0, 1000), (25, 64), (1000, 33)):
        check_invariants(len(seq), rows, gap, window)
        loci = ribbit_amd.host_record_loci(len(seq), rows, gap)
        assert 0 < len(loci) < len(rows) and loci["rows"].max() >= 2
        text = ribbit_amd.bed_loci_text(name, bed, loci)
        assert text.decode() == loci_contract.loci_lines(name, bed, loci.tolist())
        for line, l in zip(text.decode().splitlines(), loci.tolist()):
            cols = line.split("\t")
            assert len(cols) == 16 and cols[:2] == ["chr", "X"]          # 15 columns and the name's own tab
            assert l[0] <= int(cols[6]) and int(cols[7]) <= l[1]          # the best row lies in its locus
    assert ribbit_amd.bed_loci_text(name, bed, np.zeros(0, ribbit_amd.LOCUS_DT)) == b""
    assert ribbit_amd.bed_loci_text("", "", []) == b""
    # a last row without its newline is still a row
    loci = ribbit_amd.host_record_loci(len(seq), rows, 0)
    assert ribbit_amd.bed_loci_text(name, bed[:-1], loci) == ribbit_amd.bed_loci_text(name, bed, loci)
    bad = loci.copy()
    bad["best_row"][len(bad) // 2] = len(rows)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_loci_text(name, bed, bad)
    bad["best_row"][len(bad) // 2] = -1
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_loci_text(name, bed, bad)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.bed_loci_text(name, "a\t1\t2\n" * len(rows), loci)


def test_loci_text_of_a_chromosome_sized_bed():
    """tens of megabytes of rows (line starts found and lines written in pieces on several threads)"""
    rs = np.random.RandomState(6)
    n = 300_000
    starts = np.sort(rs.randint(0, 1 << 30, n))
    ends = starts + rs.randint(1, 3000, n)
    cigars = ["".join(f"{rs.randint(1, 40)}=" for _ in range(rs.randint(1, 12))) for _ in range(97)]
    order = rs.permutation(n)
    lines = [f"chr\t{starts[i]}\t{ends[i]}\tACG\t3 | 3\t{ends[i] - starts[i]}\t4\t0.9\t+\tSEED-5\t{cigars[i % 97]}\n" for i in order]
    bed = "".join(lines)
    assert len(bed) > 12 << 20
    rows = ribbit_amd.bed_intervals(bed)
    loci = ribbit_amd.host_record_loci(1 << 30, rows, 0)
    assert 50_000 < len(loci) < n and (np.diff(loci["start"]) > 0).all() and loci["rows"].sum() == n
    text = ribbit_amd.bed_loci_text("chr", bed, loci).decode().splitlines(keepends=True)
    assert len(text) == len(loci)
    for k in list(range(0, len(loci), 997)) + [len(loci) - 1]:
        l = loci[k]
        assert text[k] == f"chr\t{l['start']}\t{l['end']}\t{l['rows']}\t{l['covered']}\t" + lines[l["best_row"]].split("\t", 1)[1]


def test_bad_arguments_rejected(hip_lib):
    loci, cov, text, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
    iv = (C.c_int32 * 2)(0, 3)
    L = hip_lib
    assert L.ribbit_host_record_loci(10, iv, 1, -1, C.byref(loci), C.byref(n)) == -1
    assert b"gap" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_loci(10, None, 1, 0, C.byref(loci), C.byref(n)) == -1
    assert L.ribbit_host_record_loci(10, iv, 1, 0, None, C.byref(n)) == -1
    assert L.ribbit_host_record_loci(10, iv, 1, 0, C.byref(loci), None) == -1
    assert L.ribbit_host_record_loci(-1, iv, 1, 0, C.byref(loci), C.byref(n)) == -1
    assert L.ribbit_host_record_loci(1 << 31, iv, 1, 0, C.byref(loci), C.byref(n)) == -1
    assert L.ribbit_host_record_loci(10, None, 0, 0, C.byref(loci), C.byref(n)) == 0 and n.value == 0
    L.ribbit_loci_free(loci)
    assert L.ribbit_host_record_density(10, iv, 1, 0, C.byref(cov), C.byref(n)) == -1
    assert b"window" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_density(10, iv, 1, -5, C.byref(cov), C.byref(n)) == -1
    assert L.ribbit_host_record_density(10, None, 1, 5, C.byref(cov), C.byref(n)) == -1
    assert L.ribbit_host_record_density(10, iv, 1, 5, None, C.byref(n)) == -1
    assert L.ribbit_host_record_density(10, iv, 1, 5, C.byref(cov), None) == -1
    assert L.ribbit_host_record_density(10, None, 0, 4, C.byref(cov), C.byref(n)) == 0 and n.value == 3
    L.ribbit_intervals_free(cov)
    # a null handle is refused before anything else (no GPU needed to say so)
    assert L.ribbit_hip_record_loci(None, iv, 1, 0, C.byref(loci), C.byref(n)) == -1
    assert L.ribbit_hip_record_density(None, iv, 1, 10, C.byref(cov), C.byref(n)) == -1
    assert L.ribbit_bed_loci_text(None, b"", 0, None, 0, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_loci_text(b"a", None, 5, None, 0, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_loci_text(b"a", b"", 0, None, 1, C.byref(text), C.byref(n)) == -1
    assert L.ribbit_bed_loci_text(b"a", b"", 0, None, 0, None, C.byref(n)) == -1
    with pytest.raises(ValueError):
        ribbit_amd.host_record_loci(10, [(0, 3)], 1 << 31)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
        ribbit_amd.host_record_density(10, [(0, 3)], 0)


def test_new_files_are_part_of_every_build():
    """loci.hip and api_loci.cpp are in the Makefile's NAMES: the sanitizer builds instrument the new host code too"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [l for l in open(os.path.join(root, "ribbit_amd", "csrc", "Makefile")) if l.startswith("NAMES")][0].split()
    assert "loci" in names and "api_loci" in names


BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ribbit_amd", "ribbit-hip")


@pytest.mark.parametrize("args,option", [(["--loci-gap", "5"], "--loci-gap"),
                                         (["--density-window", "100"], "--density-window"),
                                         (["--loci-bed", "{out}", "--loci-gap", "-1"], "--loci-gap"),
                                         (["--loci-bed", "{out}", "--loci-gap", "5x"], "--loci-gap"),
                                         (["--density-bedgraph", "{out}", "--density-window", "0"], "--density-window"),
                                         (["--density-bedgraph", "{out}", "--density-window", "-3"], "--density-window"),
                                         (["--density-bedgraph", "{out}", "--density-window", "1e4"], "--density-window"),
                                         (["--loci-bed", "{out}", "--loci-gap", "2147483648"], "--loci-gap")])
def test_cli_rejects_bad_loci_options_before_any_gpu(tmp_path, args, option):
    """checked while the arguments are parsed: exit 1, the option named, no GPU opened (this runs without one)"""
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">a\nACGTACGT\n")
    argv = [BIN, "-i", str(fa)] + [a.format(out=tmp_path / "out.txt") for a in args]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert option in r.stderr and "GPU" not in r.stderr, r.stderr


def test_cli_help_says_what_the_density_counts():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    for option in ("--loci-bed", "--loci-gap", "--density-bedgraph", "--density-window"):
        assert option in r.stderr
    assert "not a fraction" in r.stderr
