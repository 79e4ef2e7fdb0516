"""The best non-overlapping rows on the GPU (best.hip through ribbit_hip_record_best): Scanner.record_best against the host twin and
the plain-Python statement of the contract (tests/best_contract.py), and ribbit-hip --best-bed end to end."""
import numpy as np
import pytest

import best_contract
import ribbit_amd
import segments
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 2048, 4100)
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)      # the wave and block edges of the lane-per-row kernels


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _same(sc, length, iv, contract=True):
    rows, bases = sc.record_best(iv)
    assert rows.dtype == np.int32
    host_rows, host_bases = ribbit_amd.host_record_best(length, iv)
    assert (rows.tolist(), bases) == (host_rows.tolist(), host_bases), length
    if contract:
        assert (rows.tolist(), bases) == best_contract.record_best(length, iv), length
    return rows.tolist(), bases


def test_edge_lengths_sets_and_row_counts():
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in LENGTHS:
            sc.load_record(_seq(length, length + 1))
            for iv in best_contract.edge_case_sets(length):
                chosen, bases = _same(sc, length, iv)
                best_contract.check_properties(length, iv, chosen, bases)
            for n in ROW_COUNTS if length >= 300 else ():
                # every row non-empty: overlapping neighbours, in an order that is not the sorted one
                full = [((37 * i) % n * 3 % (length - 9), (37 * i) % n * 3 % (length - 9) + 4 + i % 6) for i in range(n)]
                assert len(_same(sc, length, full)[0]) > 0
                # every other row empty: the all-ones keys are the sort's tail
                holes = [row if i % 2 == 0 else (row[1], row[0]) for i, row in enumerate(full)]
                chosen, bases = _same(sc, length, holes)
                best_contract.check_properties(length, holes, chosen, bases)
                assert all(i % 2 == 0 for i in chosen) and (n == 1 or len(chosen) < n)


def test_random_records():
    rs = np.random.RandomState(77)
    with ribbit_amd.Scanner(2, 30) as sc:
        for t in range(40):
            length, iv = best_contract.random_record(rs, t)
            sc.load_record(_seq(length, t))
            chosen, bases = _same(sc, length, iv)
            best_contract.check_properties(length, iv, chosen, bases)


def test_ties_go_to_the_lowest_index_whatever_the_order():
    rows = [(100, 130), (90, 120), (110, 140), (95, 100), (300, 310), (301, 311), (299, 309), (302, 303)]
    rs = np.random.RandomState(3)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(400, 1))
        chosen, bases = _same(sc, 400, rows)
        assert bases == 45
        for _ in range(20):
            shuffled = [rows[i] for i in rs.permutation(len(rows))]
            got, got_bases = _same(sc, 400, shuffled)
            assert ([shuffled[i] for i in got], got_bases) == ([rows[i] for i in chosen], bases)
        assert _same(sc, 400, [(20, 30)] * 5 + [(100, 130)] * 3) == ([0, 5], 40)


def test_one_long_segment():
    """a single lane walks everything: a chain in which every row overlaps the next, the chain nested in one row, copies of one row"""
    n = 20_000
    length = 10 * (n - 1) + 15 + 10
    chain = np.stack([10 * np.arange(n), 10 * np.arange(n) + 15], 1)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(b"ACGT" * (length // 4) + b"A" * (length % 4))
        assert length == 200_015
        chosen, bases = _same(sc, length, chain)
        assert (chosen, bases) == (list(range(0, n, 2)), 15 * n // 2)
        perm = np.random.RandomState(2).permutation(n)
        chosen, bases = _same(sc, length, chain[perm])
        assert (perm[chosen].tolist(), bases) == (list(range(0, n, 2)), 15 * n // 2)
        nested = np.concatenate([chain[: n // 2], [[0, length]], chain[n // 2:]])
        assert _same(sc, length, nested) == ([n // 2], length)
        assert _same(sc, length, np.tile([[1234, 5678]], (n, 1))) == ([0], 5678 - 1234)


def test_many_short_segments():
    """every sorted position is a segment head: disjoint rows; then more rows than one launch has lanes (1024 blocks of 256), short
    ones that overlap a few neighbours, some empty or out of range: the lanes of the first blocks take a second turn"""
    n = 100_000
    rows = np.stack([10 * np.arange(n), 10 * np.arange(n) + 5], 1)
    perm = np.random.RandomState(4).permutation(n)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(b"ACGT" * (10 * n // 4))
        assert _same(sc, 10 * n, rows, contract=False) == (list(range(n)), 5 * n)
        chosen, bases = _same(sc, 10 * n, rows[perm])
        assert (perm[chosen].tolist(), bases) == (list(range(n)), 5 * n)
        rs = np.random.RandomState(17)
        starts = rs.randint(-20, 10 * n + 20, 1024 * 256 + 65)
        wide = np.stack([starts, starts + rs.randint(-3, 40, len(starts))], 1)
        chosen, bases = _same(sc, 10 * n, wide, contract=False)
        best_contract.check_properties(10 * n, wide, chosen, bases)


def test_the_same_handle_twice_and_a_new_record():
    """nothing of a call shows through in the next: fewer rows after many, other rows of the same number, a shorter record"""
    rs = np.random.RandomState(9)
    starts = rs.randint(-50, 30_050, 3000)
    many = np.stack([starts, starts + rs.randint(-5, 400, 3000)], 1)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(30_000))
        first = _same(sc, 30_000, many)
        _same(sc, 30_000, many[:70])
        _same(sc, 30_000, many[::-1])
        _same(sc, 30_000, [(5, 9)])
        assert _same(sc, 30_000, []) == ([], 0)
        assert _same(sc, 30_000, [(9, 5), (40_000, 50_000)]) == ([], 0)
        assert _same(sc, 30_000, many) == first
        sc.load_record(_seq(9_000, 1))
        assert _same(sc, 9_000, many) != first
        sc.load_record(_seq(0))
        assert _same(sc, 0, many) == ([], 0)
        sc.load_record(_seq(30_000))
        assert _same(sc, 30_000, many) == first


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_best([(0, 1)])


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    length = len(seq)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        rows = ribbit_amd.bed_intervals(sc.refine_bed("chr"))
        assert len(rows) > 50_000
        giants = np.array([[1_000_003, 1_013_000], [2_500_000, 2_620_001], [7_990_000, 8_100_000]], np.int32)
        iv = np.concatenate([rows, giants])
        iv = iv[np.random.RandomState(1).permutation(len(iv))]
        chosen, bases = _same(sc, length, iv, contract=False)
        best_contract.check_properties(length, iv, chosen, bases)
        # between what the loci cover and the longest row of every locus, which is a set of rows of which no two overlap
        loci = sc.record_loci(iv, 0)
        width = np.minimum(iv[:, 1].astype(np.int64), length) - np.maximum(iv[:, 0], 0)
        assert width[loci["best_row"]].sum() <= bases <= loci["covered"].sum()
        assert len(loci) <= len(chosen) < len(iv)
        # the loci have used the handle in between; a third of the rows then
        _same(sc, length, rows[: len(rows) // 3], contract=False)


# ---- end to end
def _other_bed(fa, path):
    path.write_text("".join(f"{name}\t{k * 997}\t{k * 997 + 400}\n" for name, bases in records(fa) if name for k in range(len(bases) // 2000)))


def _expected(fa, bed):
    """the file: per record, in input order, what ribbit_bed_rows_text makes of the host twin's selection from the record's BED rows"""
    by_name = rows_by_record(bed)
    text = b""
    for name, bases in records(fa):
        rows = by_name.get(name, "")
        chosen, _ = ribbit_amd.host_record_best(len(bases), ribbit_amd.bed_intervals(rows))
        text += ribbit_amd.bed_rows_text(rows, chosen)
    return text.decode()


def test_cli_best_bed(tmp_path):
    fa, other = tmp_path / "in.fa", tmp_path / "other.bed"
    write_nine_records(fa, 300, 77)
    _other_bed(fa, other)
    common = ["-i", fa, "-m", 2, "-M", 30]
    bed0 = tmp_path / "plain.bed"
    _run(common + ["-o", bed0, "--loci-bed", tmp_path / "plain.loci.bed", "--timing", tmp_path / "t0.json"])
    want_bed = bed0.read_text()
    assert "best" not in _stages(tmp_path / "t0.json")
    want = _expected(fa, want_bed)
    bed_lines = set(want_bed.splitlines())
    assert 0 < len(want.splitlines()) < len(want_bed.splitlines()) and all(line in bed_lines for line in want.splitlines())
    for name, text in rows_by_record(want).items():      # per record: sorted by start, no two rows overlap
        iv = ribbit_amd.bed_intervals(text)
        assert (iv[1:, 0] >= iv[:-1, 1]).all(), name
    seven = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary"]
    runs = [[], ["--jobs", "3"], ["--devices", "0,0", "--jobs", "2"],
            ["--overlap-with", other] + [x for k, option in enumerate(seven) for x in (option, tmp_path / f"other{k}")]]
    for k, extra in enumerate(runs):
        bed, best, timing = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.best.bed", tmp_path / f"t{k + 1}.json"
        _run(common + ["-o", bed, "--best-bed", best, "--timing", timing] + extra)
        assert bed.read_text() == want_bed
        assert best.read_text() == want, extra
        assert list(_stages(timing))[-1] == "best"
    assert list(_stages(tmp_path / "t4.json"))[6:] == ["mask", "repeats", "loci", "density", "overlap", "best"]
    assert (tmp_path / "other2").read_text() == (tmp_path / "plain.loci.bed").read_text()
