"""The masked FASTA on the GPU (mask.hip through ribbit_hip_mask_record): Scanner.mask_record against the host twin and
the numpy statement of the contract (tests/mask_contract.py), and ribbit-hip --masked-fasta end to end."""
import numpy as np
import pytest

import ribbit_amd
import segments
from mask_contract import masked_body
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence, write_fasta

pytestmark = pytest.mark.gpu
MODES = ("soft", "hard")


def _seq(n, seed):
    return np.frombuffer(b"ACGTNacgtRY\r", np.uint8)[np.random.RandomState(seed).randint(0, 12, n)].tobytes()


def _same(sc, seq, iv, mode, width):
    got = sc.mask_record(iv, mode, width)
    assert got == ribbit_amd.host_mask_record(seq, iv, mode, width), (len(seq), mode, width)
    assert got == masked_body(seq, iv, mode, width), (len(seq), mode, width)


def test_edge_cases_match_host_twin_and_contract():
    with ribbit_amd.Scanner(2, 30) as sc:
        for length, width in [(0, 60), (0, 0), (7, 60), (120, 60), (180, 60), (37, 1), (1, 1), (95, 0), (64, 64), (65, 64), (100, 3),
                              (300, 16), (300, 15), (300, 17)] + [(n, w) for n in (15, 16, 17, 31, 32, 33, 48) for w in (60, 5)]:
            seq = _seq(length, length * 7 + width)
            sc.load_record(seq)
            sets = [[], [(0, length)], [(3, 9), (5, 20)], [(-5, 4), (length - 2, length + 50)], [(50, 10), (20, 20)],
                    [(-(1 << 31), (1 << 31) - 1)]]
            for k in (1, 2, 4):
                sets.append([(32 * k - 1, 32 * k + 1), (32 * k, 32 * k + 33), (32 * k + 1, 32 * k + 2)])
            for iv in sets:
                for mode in MODES:
                    _same(sc, seq, iv, mode, width)
        seq = bytes(range(256)) * 5
        sc.load_record(seq)
        for mode in MODES:
            _same(sc, seq, [(0, 256), (300, 700), (1000, 1280)], mode, 50)


def test_records_over_many_chunks_and_words():
    rs = np.random.RandomState(99)
    with ribbit_amd.Scanner(2, 30) as sc:
        for t in range(40):
            L = int(rs.randint(1000, 40_000))
            seq = _seq(L, t)
            sc.load_record(seq)
            n = int(rs.randint(0, 400))
            starts = rs.randint(-100, L + 100, n)
            iv = np.stack([starts, starts + rs.randint(-20, 3000, n)], 1)
            _same(sc, seq, iv, MODES[t % 2], int(rs.choice([0, 1, 2, 15, 16, 17, 60, 61, 1000, L])))


def test_unaligned_device_source():
    """bases at an odd device address (ribbit_hip_load_record_device): the edge chunks read byte by byte, the rest wide"""
    torch = pytest.importorskip("torch")
    seq = _seq(10_007, 5)
    buf = torch.zeros(len(seq) + 16, dtype=torch.uint8, device="cuda:0")
    iv = [(3, 500), (4000, 9000), (10_000, 10_007)]
    with ribbit_amd.Scanner(2, 30) as sc:
        for shift in (1, 5, 15):
            buf[shift:shift + len(seq)] = torch.frombuffer(bytearray(seq), dtype=torch.uint8).to("cuda:0")
            torch.cuda.synchronize()
            sc.load_record_device(buf.data_ptr() + shift, len(seq))
            for mode in MODES:
                _same(sc, seq, iv, mode, 61)


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    assert len(seq) >= 8_000_000
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        bed = sc.refine_bed("chr")
        rows = ribbit_amd.bed_intervals(bed)
        assert len(rows) > 50_000
        # the giants: rows of 10 kb and more, over words and chunks of every alignment (real ones when the record has any)
        giants = np.array([[1_000_003, 1_013_000], [2_500_000, 2_620_001], [7_990_000, 8_100_000]], np.int32)
        iv = np.concatenate([rows, giants])
        rs = np.random.RandomState(1)
        iv = iv[rs.permutation(len(iv))]
        got = sc.mask_record(iv, "soft", 60)
        assert got == masked_body(seq, iv, "soft", 60)
        assert got == ribbit_amd.host_mask_record(seq, iv, "soft", 60)
        # the same handle again, another width and mode: nothing of the first call may show through
        got = sc.mask_record(rows, "hard", 0)
        assert got == masked_body(seq, rows, "hard", 0)
        got = sc.mask_record(rows[: len(rows) // 3], "soft", 80)
        assert got == masked_body(seq, rows[: len(rows) // 3], "soft", 80)


def test_mask_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.mask_record([(0, 1)])


def _expected(fa, bed, mode, width):
    by_name = rows_by_record(bed)
    return b"".join(b">" + n.encode() + b"\n" + masked_body(b, ribbit_amd.bed_intervals(by_name.get(n, "")), mode, width) for n, b in records(fa))


def test_cli_masked_fasta(tmp_path):
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 300, 77)

    bed0 = tmp_path / "plain.bed"
    _run(["-i", fa, "-o", bed0, "-m", 2, "-M", 30, "--timing", tmp_path / "t0.json"])
    want_bed = bed0.read_text()
    assert "mask" not in _stages(tmp_path / "t0.json")
    runs = [("soft", 60, []), ("hard", 0, ["--mask", "hard", "--mask-width", "0"]),
            ("soft", 7, ["--mask", "soft", "--mask-width", "7", "--devices", "0,0", "--jobs", "2"])]
    for k, (mode, width, extra) in enumerate(runs):
        bed, out = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.fa"
        _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--masked-fasta", out, "--timing", tmp_path / f"t{k}.json"] + extra)
        assert bed.read_text() == want_bed
        assert out.read_bytes() == _expected(fa, want_bed, mode, width), (mode, width, extra)
        assert "mask" in _stages(tmp_path / f"t{k}.json")


def test_cli_masked_fasta_refined_in_slices(tmp_path):
    """one record refined in slices over three handles: its mask is the union of all slices' rows"""
    recs = [("small", simulate_sequence(30_000, 11, 2, 30, lower_rate=0.2)[0]),
            ("big", simulate_sequence(400_000, 12, 2, 30, n_block_rate=0.2, lower_rate=0.2)[0])]
    fa, bed0, bed, out = tmp_path / "in.fa", tmp_path / "plain.bed", tmp_path / "out.bed", tmp_path / "out.fa"
    write_fasta(str(fa), recs)
    _run(["-i", fa, "-o", bed0, "-m", 2, "-M", 30])
    r = _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--devices", "0,0,0", "--masked-fasta", out, "--mask", "hard"],
             env={"RIBBIT_SHARD_MIN_SEEDS": "100", "RIBBIT_PROFILE": "1"})
    assert "[devices] refinement of big:" in r.stderr and "seeds in 3 slices" in r.stderr, r.stderr[-1500:]
    assert bed.read_text() == bed0.read_text()
    assert out.read_bytes() == _expected(fa, bed0.read_text(), "hard", 60)
    assert sum(l.startswith("big\t") for l in bed0.read_text().splitlines()) > 30
