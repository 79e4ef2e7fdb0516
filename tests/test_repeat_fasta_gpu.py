"""The repeat FASTA on the GPU (repeats.hip through ribbit_hip_repeat_sequences): Scanner.repeat_sequences against the host
twin and the numpy statement of the contract (tests/repeat_contract.py), in batches of forced text budgets, and ribbit-hip
--repeat-fasta end to end."""
import numpy as np
import pytest

import ribbit_amd
import segments
from mask_contract import masked_body
from repeat_contract import repeat_entries
from cli_rows import records as _records, rows_by_record as _rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence, write_fasta
from test_repeat_fasta import I32_MAX, edge_rows

pytestmark = pytest.mark.gpu


def _seq(n, seed):
    return np.frombuffer(b"ACGTNacgtRY\r", np.uint8)[np.random.RandomState(seed).randint(0, 12, n)].tobytes()


def _same(sc, name, seq, iv, flank):
    got = sc.repeat_sequences(name, iv, flank)
    assert got == ribbit_amd.host_repeat_sequences(name, seq, iv, flank), (len(seq), flank)
    assert got == repeat_entries(name, seq, iv, flank), (len(seq), flank)
    return got


def test_edge_cases_match_host_twin_and_contract():
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 300):
            seq = _seq(length, length + 3)
            sc.load_record(seq)
            for flank in (0, 1, 100, length, length + 1, I32_MAX):
                for name in ("chr1", "", "a:b\tc"):
                    _same(sc, name, seq, edge_rows(length), flank)
            _same(sc, "one", seq, [(1, 0)], 5)
            assert sc.repeat_sequences("none", [], 5) == b""
        seq = bytes(range(256)) * 5
        sc.load_record(seq)
        for flank in (0, 3, 100):
            _same(sc, "bytes", seq, [(0, 256), (300, 700), (1000, 1280), (17, 17)], flank)


def test_records_with_random_rows():
    rs = np.random.RandomState(31)
    with ribbit_amd.Scanner(2, 30) as sc:
        for t in range(30):
            L = int(rs.randint(1000, 40_000))
            seq = _seq(L, t)
            sc.load_record(seq)
            n = int(rs.randint(1, 600))
            starts = rs.randint(-100, L + 100, n)
            iv = np.stack([starts, starts + rs.randint(-20, 3000, n)], 1)
            _same(sc, "r" * int(rs.randint(0, 40)), seq, iv, int(rs.choice([0, 1, 2, 15, 16, 17, 100, 1000, L])))


def test_unaligned_device_source():
    """bases at an odd device address (ribbit_hip_load_record_device): the edge windows read byte by byte, the rest wide"""
    torch = pytest.importorskip("torch")
    seq = _seq(10_007, 5)
    buf = torch.zeros(len(seq) + 16, dtype=torch.uint8, device="cuda:0")
    iv = [(3, 500), (4000, 9000), (10_000, 10_007), (0, 1), (17, 33)] + [(i, i + 7) for i in range(100, 400, 13)]
    with ribbit_amd.Scanner(2, 30) as sc:
        for shift in (1, 5, 15):
            buf[shift:shift + len(seq)] = torch.frombuffer(bytearray(seq), dtype=torch.uint8).to("cuda:0")
            torch.cuda.synchronize()
            sc.load_record_device(buf.data_ptr() + shift, len(seq))
            for flank in (0, 9, 100):
                _same(sc, "u", seq, iv, flank)


@pytest.mark.parametrize("budget", [1, 17, 4096, 0])
def test_forced_budgets(budget):
    """every batch but a one-row batch within the budget, the rows adding up to n, the text joined unchanged"""
    rs = np.random.RandomState(budget)
    seq = _seq(30_000, 8)
    starts = rs.randint(-50, len(seq) + 50, 700)
    iv = np.stack([starts, starts + rs.randint(-5, 200, len(starts))], 1)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        sc.debug_set_repeat_text_budget(budget)
        for flank in (0, 30, 2000):
            want = repeat_entries("chrB", seq, iv, flank)
            batches = sc.repeat_sequence_batches("chrB", iv, flank)
            assert b"".join(t for t, _ in batches) == want
            assert sum(k for _, k in batches) == len(iv)
            limit = budget or 64 << 20
            assert all(len(t) <= limit or k == 1 for t, k in batches)
            if budget == 1:
                assert all(k == 1 for _, k in batches)
            if budget == 4096 and flank == 0:
                assert len(batches) > 1 and all(len(t) + 250 > 4096 for t, _ in batches[:-1])
        sc.debug_set_repeat_text_budget(0)
        assert sc.repeat_sequences("chrB", iv, 30) == repeat_entries("chrB", seq, iv, 30)


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        rows = ribbit_amd.bed_intervals(sc.refine_bed("chr"))
        assert len(rows) > 50_000
        for flank in (0, 100, 5000):
            got = sc.repeat_sequences("chr", rows, flank)
            assert got == repeat_entries("chr", seq, rows, flank), flank
            if flank == 100:
                assert got == ribbit_amd.host_repeat_sequences("chr", seq, rows, flank)


def test_repeat_sequences_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.repeat_sequences("c", [(0, 1)])
        sc.load_record(b"ACGT" * 10)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            sc.repeat_sequences("c", [(0, 1)], -1)


def _expected_repeats(fa, bed, flank):
    by_name = _rows_by_record(bed)
    return b"".join(repeat_entries(n, b, ribbit_amd.bed_intervals(by_name.get(n, "")), flank) for n, b in _records(fa))


def _expected_masked(fa, bed):
    by_name = _rows_by_record(bed)
    return b"".join(b">" + n.encode() + b"\n" + masked_body(b, ribbit_amd.bed_intervals(by_name.get(n, "")), "soft", 60)
                    for n, b in _records(fa))


def test_cli_repeat_fasta(tmp_path):
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 400, 78)

    bed0 = tmp_path / "plain.bed"
    _run(["-i", fa, "-o", bed0, "-m", 2, "-M", 30, "--timing", tmp_path / "t0.json"])
    want_bed = bed0.read_text()
    assert "repeats" not in _stages(tmp_path / "t0.json")
    assert len(want_bed.splitlines()) > 100
    runs = [(100, [], False), (7, ["--flank", "7", "--masked-fasta", "{m}"], True), (0, ["--flank", "0", "--devices", "0,0", "--jobs", "2"], False),
            (1000, ["--flank=1000", "--jobs", "3", "--masked-fasta", "{m}"], True)]
    for k, (flank, extra, masked) in enumerate(runs):
        bed, out, m = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.fa", tmp_path / f"m{k}.fa"
        _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--repeat-fasta", out, "--timing", tmp_path / f"t{k}.json"]
             + [a.format(m=m) for a in extra])
        assert bed.read_text() == want_bed
        assert out.read_bytes() == _expected_repeats(fa, want_bed, flank), extra
        stages = _stages(tmp_path / f"t{k}.json")
        assert "repeats" in stages and ("mask" in stages) == masked
        if masked:
            assert m.read_bytes() == _expected_masked(fa, want_bed)


def test_cli_repeat_fasta_refined_in_slices(tmp_path):
    """one record refined in slices over three handles: its entries follow the rows of all slices in BED order"""
    recs = [("small", simulate_sequence(30_000, 21, 2, 30, lower_rate=0.2)[0]),
            ("big", simulate_sequence(400_000, 22, 2, 30, n_block_rate=0.2, lower_rate=0.2)[0])]
    fa, bed0, bed, out, m = tmp_path / "in.fa", tmp_path / "plain.bed", tmp_path / "out.bed", tmp_path / "out.fa", tmp_path / "m.fa"
    write_fasta(str(fa), recs)
    _run(["-i", fa, "-o", bed0, "-m", 2, "-M", 30])
    r = _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--devices", "0,0,0", "--repeat-fasta", out, "--flank", "50", "--masked-fasta", m],
             env={"RIBBIT_SHARD_MIN_SEEDS": "100", "RIBBIT_PROFILE": "1"})
    assert "[devices] refinement of big:" in r.stderr and "seeds in 3 slices" in r.stderr, r.stderr[-1500:]
    assert "  repeats " in r.stderr
    assert bed.read_text() == bed0.read_text()
    assert out.read_bytes() == _expected_repeats(fa, bed0.read_text(), 50)
    assert m.read_bytes() == _expected_masked(fa, bed0.read_text())
    assert sum(l.startswith("big\t") for l in bed0.read_text().splitlines()) > 30
