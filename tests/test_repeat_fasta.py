"""The repeat FASTA without a GPU: ribbit_host_repeat_sequences against the numpy statement of the contract
(tests/repeat_contract.py), its argument checks, and the command line's checks of --repeat-fasta / --flank."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ribbit_amd
from repeat_contract import repeat_entries

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")


def _seq(n, seed):
    return np.frombuffer(b"ACGTNacgtRY\r", np.uint8)[np.random.RandomState(seed).randint(0, 12, n)].tobytes()


def _check(name, seq, iv, flank):
    got = ribbit_amd.host_repeat_sequences(name, seq, iv, flank)
    assert got == repeat_entries(name, seq, iv, flank), (len(seq), flank)
    return got


def edge_rows(L):
    """rows at 0 and L, reversed, empty, outside the record and at the int32 extremes"""
    return [(0, 0), (0, 1), (0, L), (L, L), (L - 1, L), (max(L - 1, 0), L + 5), (5, 2), (3, 3), (-10, -1), (L + 1, L + 9),
            (-7, 4), (I32_MIN, I32_MAX), (I32_MAX, I32_MAX), (I32_MIN, I32_MIN), (I32_MAX, I32_MIN), (L // 2, L // 2 + 3)]


@pytest.mark.parametrize("length", [0, 1, 15, 16, 17, 300])
def test_edge_rows_and_flanks(length):
    seq = _seq(length, length)
    for flank in (0, 1, 100, length, length + 1, I32_MAX):
        _check("chr1", seq, edge_rows(length), flank)


@pytest.mark.parametrize("name", ["", "a", "chr:1-5", "with\ttab", "x" * 300])
def test_names(name):
    seq = _seq(120, 4)
    got = _check(name, seq, [(10, 20), (100, 130)], 7)
    assert got.startswith(b">" + name.encode() + b":10-20 flank=7,7\n")


def test_all_byte_values():
    seq = bytes(range(256)) * 3
    got = _check("b", seq, [(0, 256), (300, 700), (10, 10)], 40)
    first = got.split(b"\n", 1)[1][:296]
    assert first == seq[:296]


def test_entry_shape():
    seq = b"ACGTACGTACGTAC"
    got = ribbit_amd.host_repeat_sequences("chr", seq, [(2, 5), (12, 20), (9, 3), (-4, -1)], 3)
    assert got == (b">chr:2-5 flank=2,3\nACGTACGT\n>chr:12-14 flank=3,0\nCGTAC\n"
                   b">chr:9-9 flank=3,3\nGTACGT\n>chr:0-0 flank=0,3\nACG\n")
    assert ribbit_amd.host_repeat_sequences("chr", seq, [], 3) == b""
    assert ribbit_amd.host_repeat_sequences("chr", b"", [(0, 5)], 3) == b">chr:0-0 flank=0,0\n\n"


def test_random_row_sets():
    rs = np.random.RandomState(77)
    for t in range(40):
        L = int(rs.choice([1, 16, 17, 200, 1000, rs.randint(0, 5000)]))
        seq = _seq(L, t)
        n = int(rs.randint(0, 60))
        starts = rs.randint(-50, L + 50, n)
        iv = np.stack([starts, starts + rs.randint(-30, 400, n)], 1) if n else np.zeros((0, 2), int)
        _check(f"r{t}", seq, iv, int(rs.choice([0, 1, 2, 50, 100, L, L + 1, I32_MAX])))


def test_bad_arguments_rejected(hip_lib):
    text, n = C.c_void_p(), C.c_size_t()
    iv = (C.c_int32 * 2)(0, 3)
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, iv, 1, -1, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_repeat_sequences(None, b"ACGT", 4, iv, 1, 5, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, None, 1, 5, C.byref(text), C.byref(n)) == -1
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, iv, 1, 5, None, C.byref(n)) == -1
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, iv, 1, 5, C.byref(text), None) == -1
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, None, 0, 5, C.byref(text), C.byref(n)) == 0
    assert n.value == 0
    hip_lib.ribbit_text_free(text)
    assert hip_lib.ribbit_host_repeat_sequences(b"c", b"ACGT", 4, iv, 1, 1, C.byref(text), C.byref(n)) == 0
    assert C.string_at(text.value, n.value) == b">c:0-3 flank=0,1\nACGT\n"
    hip_lib.ribbit_text_free(text)
    with pytest.raises(ribbit_amd.RibbitHipError):
        ribbit_amd.host_repeat_sequences("c", b"ACGT", [(0, 3)], -1)
    with pytest.raises(ValueError):
        ribbit_amd.host_repeat_sequences("c", b"ACGT", [(0, 3)], I32_MAX + 1)


def test_gpu_entry_point_checks_its_arguments_first(hip_lib):
    """the GPU form refuses bad arguments before it looks at the handle (this runs without a GPU)"""
    fn = hip_lib.ribbit_hip_repeat_sequences
    text, n, k = C.c_void_p(), C.c_size_t(), C.c_size_t()
    iv = (C.c_int32 * 2)(0, 3)
    assert fn(None, b"c", iv, 1, 5, C.byref(text), C.byref(n), C.byref(k)) == -1
    assert hip_lib.ribbit_hip_debug_set_repeat_text_budget(None, 10) == -1


@pytest.mark.parametrize("args,option", [(["--repeat-fasta", "{out}", "--flank", "-1"], "--flank"),
                                         (["--repeat-fasta", "{out}", "--flank", "1x"], "--flank"),
                                         (["--repeat-fasta", "{out}", "--flank", ""], "--flank"),
                                         (["--repeat-fasta", "{out}", "--flank", "1234567890"], "--flank"),
                                         (["--flank", "10"], "--flank"),
                                         (["--repeat-fasta", ""], "--repeat-fasta"),
                                         (["--repeat-fasta", "{missing}"], "--repeat-fasta")])
def test_cli_rejects_bad_repeat_options_before_any_gpu(tmp_path, args, option):
    """checked while the arguments are parsed: exit 1, the option named, no GPU opened (this runs without one)"""
    fa = tmp_path / "in.fa"
    fa.write_bytes(b">a\nACGTACGT\n")
    argv = [BIN, "-i", str(fa)] + [a.format(out=tmp_path / "r.fa", missing=tmp_path / "no" / "such" / "r.fa") for a in args]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert option in r.stderr and "GPU" not in r.stderr, r.stderr


def test_cli_help_lists_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert "--repeat-fasta" in r.stderr and "--flank" in r.stderr
