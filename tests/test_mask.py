"""The masked FASTA body without a GPU: ribbit_host_mask_record and ribbit_bed_intervals against the numpy statement of
the contract (tests/mask_contract.py)."""
import os
import subprocess

import numpy as np
import pytest

import ribbit_amd
from cases import simulated_cases
from mask_contract import masked_body
from oracle_lib import Oracle

MODES = ("soft", "hard")


def _check(seq, intervals, mode, width):
    got = ribbit_amd.host_mask_record(seq, intervals, mode, width)
    assert got == masked_body(seq, intervals, mode, width), (len(seq), mode, width)
    return got


def _acgt(n, seed):
    return np.frombuffer(b"ACGTNacgtRY", np.uint8)[np.random.RandomState(seed).randint(0, 11, n)].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("length,width", [(0, 60), (0, 0), (7, 60), (120, 60), (180, 60), (37, 1), (1, 1), (95, 0), (64, 64),
                                          (65, 64), (100, 3)])
def test_lengths_and_widths(length, width, mode):
    seq = _acgt(length, length + width)
    for iv in ([], [(0, length)], [(3, 9), (5, 20)], [(-5, 4), (length - 2, length + 50)]):
        _check(seq, iv, mode, width)


@pytest.mark.parametrize("mode", MODES)
def test_interval_shapes(mode):
    seq = _acgt(300, 7)
    cases = {
        "empty": [],
        "overlapping": [(10, 50), (40, 90), (45, 46), (10, 50)],
        "unsorted": [(200, 220), (5, 9), (100, 101), (60, 70)],
        "out of range": [(-100, -1), (300, 400), (-7, 3), (299, 1000), (-(1 << 31), (1 << 31) - 1)],
        "reversed": [(50, 10), (20, 20), (90, -5)],
        "whole record": [(0, 300)],
    }
    for name, iv in cases.items():
        got = _check(seq, iv, mode, 60)
        if name == "reversed" or name == "empty":
            assert got == masked_body(seq, [], mode, 60)
    assert _check(seq, [(-(1 << 31), (1 << 31) - 1)], "hard", 0) == b"N" * 300 + b"\n"


@pytest.mark.parametrize("mode", MODES)
def test_bitmap_word_boundaries(mode):
    seq = _acgt(32 * 9 + 5, 3)
    for k in (1, 2, 4, 8):
        for s in (32 * k - 1, 32 * k, 32 * k + 1):
            for e in (s + 1, 32 * k + 31, 32 * k + 32, 32 * k + 33, 32 * (k + 1) - 1):
                _check(seq, [(s, e)], mode, 60)
                _check(seq, [(0, s), (e, len(seq))], mode, 17)


@pytest.mark.parametrize("mode", MODES)
def test_all_byte_values(mode):
    seq = bytes(range(256)) * 3
    masked = [(0, 256), (300, 512)]
    _check(seq, masked, mode, 50)
    body = np.frombuffer(_check(seq, masked, mode, 0)[:-1], np.uint8)
    assert len(body) == len(seq)
    src = np.frombuffer(seq, np.uint8)
    cov = np.zeros(len(seq), bool)
    cov[0:256] = cov[300:512] = True
    assert (body[~cov] == src[~cov]).all()
    if mode == "hard":
        assert (body[cov] == ord("N")).all()
    else:
        letters = (src >= 65) & (src <= 90)
        assert (body[cov & letters] == src[cov & letters] + 32).all()
        assert (body[cov & ~letters] == src[cov & ~letters]).all()


def test_random_interval_sets():
    rs = np.random.RandomState(2024)
    for t in range(300):
        L = int(rs.choice([1, 31, 33, 200, 1000, rs.randint(0, 5000)]))
        seq = _acgt(L, t)
        n = rs.randint(0, 40)
        iv = np.stack([rs.randint(-50, L + 50, n), rs.randint(-50, L + 50, n)], 1) if n else np.zeros((0, 2), int)
        long = rs.randint(0, L + 1, 2) if L else (0, 0)
        iv = np.concatenate([iv, [sorted(long)]]) if rs.rand() < 0.5 else iv
        _check(seq, iv, MODES[t % 2], int(rs.choice([0, 1, 7, 60, 61, 80, L + 3])))


def test_bad_arguments_rejected(hip_lib):
    import ctypes as C
    text, n = C.c_void_p(), C.c_size_t()
    iv = (C.c_int32 * 2)(0, 3)
    assert hip_lib.ribbit_host_mask_record(b"ACGT", 4, iv, 1, 2, 60, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_mask_record(b"ACGT", 4, iv, 1, 0, -1, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_mask_record(b"ACGT", 4, None, 1, 0, 60, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_mask_record(b"ACGT", 4, None, 0, 1, 60, C.byref(text), C.byref(n)) == 0
    assert C.string_at(text.value, n.value) == b"ACGT\n"
    hip_lib.ribbit_text_free(text)
    with pytest.raises(ValueError):
        ribbit_amd.host_mask_record(b"ACGT", [], "lower")


def test_bed_intervals_of_oracle_rows():
    seq = simulated_cases()[0][1][:40_000]
    with Oracle(seq, 2, 30) as o:
        o.run_all()
        bed = o.refine_bed("chr\tX")          # (a name with a tab in it: the columns are read from the right)
    rows = [l.split("\t") for l in bed.splitlines()]
    assert len(rows) > 100
    got = ribbit_amd.bed_intervals(bed)
    assert got.dtype == np.int32 and got.shape == (len(rows), 2)
    assert got.tolist() == [[int(r[-10]), int(r[-9])] for r in rows]
    assert (got[:, 1] - got[:, 0] == np.array([int(r[-6]) for r in rows])).all()      # column 6: length = end - start
    assert ribbit_amd.bed_intervals("").shape == (0, 2)
    assert ribbit_amd.bed_intervals(bed.encode()).tolist() == got.tolist()
    body = ribbit_amd.host_mask_record(seq, got, "soft", 60)
    assert body == masked_body(seq, got, "soft", 60)


@pytest.mark.parametrize("text", ["not a row\n", "a\t1\t2\n", "a\tx\t9\tAC\t2 | 2\t7\t3\t100\t+\tSEED-5\t7=\n",
                                  "a\t1\t99999999999\tAC\t2 | 2\t7\t3\t100\t+\tSEED-5\t7=\n",
                                  "a\t1\t9\tAC\t2 | 2\t8\t4\t100\t+\tSEED-5\t8=\n\n"])
def test_bed_intervals_rejects_what_is_not_a_row(text):
    with pytest.raises(ribbit_amd.RibbitHipError):
        ribbit_amd.bed_intervals(text)


BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ribbit_amd", "ribbit-hip")


@pytest.mark.parametrize("args,option", [(["--masked-fasta", "{out}", "--mask", "lower"], "--mask"),
                                         (["--masked-fasta", "{out}", "--mask-width", "-1"], "--mask-width"),
                                         (["--masked-fasta", "{out}", "--mask-width", "6x"], "--mask-width"),
                                         (["--mask", "hard"], "--mask"),
                                         (["--mask-width", "10"], "--mask-width")])
def test_cli_rejects_bad_mask_options_before_any_gpu(tmp_path, args, option):
    """checked while the arguments are parsed: exit 1, the option named, no GPU opened (this runs without one)"""
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">a\nACGTACGT\n")
    argv = [BIN, "-i", str(fa)] + [a.format(out=tmp_path / "m.fa") for a in args]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert option in r.stderr and "GPU" not in r.stderr, r.stderr


def test_bed_intervals_of_a_chromosome_sized_text():
    """tens of megabytes of rows (parsed in pieces on several threads): every row in order; a bad row deep inside is refused"""
    rs = np.random.RandomState(5)
    n = 400_000
    starts = rs.randint(0, 1 << 30, n)
    ends = starts + rs.randint(-5, 120_000, n)
    cigars = ["".join(f"{rs.randint(1, 40)}=" for _ in range(rs.randint(1, 12))) for _ in range(97)]
    text = "".join(f"chr\t{s}\t{e}\tACG\t3 | 3\t{e - s}\t4\t0.9\t+\tSEED-5\t{cigars[i % 97]}\n"
                   for i, (s, e) in enumerate(zip(starts, ends)))
    assert len(text) > 16 << 20
    got = ribbit_amd.bed_intervals(text)
    assert got.shape == (n, 2) and (got[:, 0] == starts).all() and (got[:, 1] == ends).all()
    lines = text.splitlines(keepends=True)
    lines[n * 3 // 4] = "chr\t12\n"
    with pytest.raises(ribbit_amd.RibbitHipError):
        ribbit_amd.bed_intervals("".join(lines))
