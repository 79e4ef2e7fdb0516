"""The rows' overlap with a second set of intervals on the GPU (overlap.hip through ribbit_hip_record_overlap):
Scanner.record_overlap against the numpy statement of the contract (tests/overlap_contract.py) and the host twin, and
ribbit-hip --overlap-with / --overlap-bed / --overlap-summary end to end."""
import numpy as np
import pytest

import overlap_contract
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages
from ribbit_amd.simulate import simulate_sequence, truth_bed_text, write_fasta

pytestmark = pytest.mark.gpu
# the word edge, a lane's block of 8 words, one wave's 64 blocks
LENGTHS = (0, 1, 31, 32, 33, 255, 256, 257, 16383, 16384, 16385)
# a launch has at most 1024 blocks of 256 lanes (overlap.hip): one stride of the block counts covers 2^26 positions, one stride
# of the interval kernels 2^18 intervals
STRIDE_LANES = 1024 * 256


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _same(sc, length, rows, other, what=None):
    per_row, totals = sc.record_overlap(rows, other)
    assert per_row.dtype == np.int32 and per_row.shape == (len(rows), 2)
    want_rows, want_totals = overlap_contract.record_overlap(length, rows, other)
    assert totals == want_totals, (length, what)
    assert per_row.tolist() == want_rows, (length, what)
    return per_row, totals


@pytest.mark.parametrize("length", LENGTHS)
def test_edge_case_sets(length):
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length, length))
        for what, rows, other in overlap_contract.edge_case_sets(length):
            per_row, totals = _same(sc, length, rows, other, what)
            host_rows, host_totals = ribbit_amd.host_record_overlap(length, rows, other)
            assert per_row.tolist() == host_rows.tolist() and totals == host_totals, what
            _same(sc, length, other, rows, what)


def test_random_sets():
    length = 100_000
    rs = np.random.RandomState(91)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length))
        for t in range(12):
            rows, other = overlap_contract.random_sets(length, rs, int(rs.randint(0, 300)), int(rs.randint(0, 300)), 60 if t % 2 else 4000)
            _same(sc, length, rows, other, t)


def test_second_call_and_new_record():
    """the same arguments again: the same result (nothing is enqueued); the same intervals after another load: that record's result;
    and the mask in between, with other rows, does not leave its bitmap to the overlap"""
    rs = np.random.RandomState(5)
    rows, other = overlap_contract.random_sets(20_000, rs, 200, 150, 700)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(20_000))
        first = _same(sc, 20_000, rows, other)
        again = sc.record_overlap(rows, other)
        assert again[0].tolist() == first[0].tolist() and again[1] == first[1]
        sc.mask_record(rows[:50], "hard", 0)
        _same(sc, 20_000, rows, other)
        _same(sc, 20_000, rows, other[:70])
        _same(sc, 20_000, rows[:90], other[:70])
        _same(sc, 20_000, rows, other)
        sc.load_record(_seq(9_000, 1))
        shorter = _same(sc, 9_000, rows, other)
        assert shorter[1] != first[1]
        sc.load_record(_seq(0))
        _same(sc, 0, rows, other)
        sc.load_record(_seq(20_000))
        assert _same(sc, 20_000, rows, other)[1] == first[1]


def _contract_without_loops(length, rows, other):
    """overlap_contract.record_overlap for sets too large for its double loop (one of the two has a few intervals): the same
    per-base arrays, read through their cumulative sums, and the pairs of clipped intervals compared all at once"""
    def clipped(iv):
        iv = np.asarray(iv, np.int64).reshape(-1, 2)
        s, e = np.clip(iv[:, 0], 0, length), np.clip(iv[:, 1], None, length)      # (a start beyond the record: an empty interval either way)
        return s, np.where(s < e, e, s)                   # (an empty interval: [s, s))
    def before(s, e):
        held = np.zeros(length, np.int64)
        for lo, hi in zip(s.tolist(), e.tolist()):
            held[lo:hi] = 1
        return np.concatenate([[0], np.cumsum(held)])
    (a_s, a_e), (b_s, b_e) = clipped(rows), clipped(other)
    a_live, b_live = a_s < a_e, b_s < b_e
    in_a, in_b = before(a_s, a_e), before(b_s, b_e)
    pairs = a_live[:, None] & b_live[None, :] & (b_s[None, :] < a_e[:, None]) & (b_e[None, :] > a_s[:, None])
    bases = in_b[a_e] - in_b[a_s]
    both = np.diff(in_a) * np.diff(in_b)
    totals = dict(rows=int(a_live.sum()), rows_hit=int((bases > 0).sum()), other=int(b_live.sum()), other_hit=int((in_a[b_e] - in_a[b_s] > 0).sum()),
                  rows_bases=int(in_a[-1]), other_bases=int(in_b[-1]), both_bases=int(both.sum()))
    return np.stack([pairs.sum(1), bases], 1).tolist(), totals


def test_sizes_beyond_one_stride():
    """more rows than one launch has lanes, then more OTHER intervals; then a record longer than one stride of the block counts"""
    rs = np.random.RandomState(17)
    length = 100_000
    many = STRIDE_LANES + 65
    starts = rs.randint(-20, length + 20, many)
    long_set = np.stack([starts, starts + rs.randint(-3, 40, many)], 1)
    few = [(100, 50_000), (49_990, 50_010), (length - 5, length + 5), (70_000, 70_000)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length))
        for rows, other in ((long_set, few), (few, long_set)):
            per_row, totals = sc.record_overlap(rows, other)
            want_rows, want_totals = _contract_without_loops(length, rows, other)
            assert totals == want_totals
            assert per_row.tolist() == want_rows
            host_rows, host_totals = ribbit_amd.host_record_overlap(length, rows, other)
            assert totals == host_totals and per_row.tolist() == host_rows.tolist()
        # a record of one stride of the block counts and a little: the lanes of the first blocks take a second turn
        length = STRIDE_LANES * 256 + 257
        sc.load_record(b"ACGT" * (length // 4) + b"A" * (length % 4))
        edge = STRIDE_LANES * 256
        rows = [(edge - 3, edge + 2), (5, 40), (edge + 200, length + 9), (1_000_000, 3_000_000), (edge + 255, edge + 257)]
        other = [(edge - 1, edge + 1), (0, 10), (length - 1, length), (2_999_999, edge + 256), (edge + 256, edge + 300)]
        _same(sc, length, rows, other, "beyond one stride")


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_overlap([(0, 1)], [(0, 1)])


# ---- end to end
def _expected(fa, bed, other_by_name):
    """the two files: the contract applied to the BED and the OTHER intervals per record, in input order"""
    by_name = rows_by_record(bed)
    overlap_bed, summary = "", ""
    for name, bases in records(fa):
        text = by_name.get(name, "")
        per_row, totals = overlap_contract.record_overlap(len(bases), ribbit_amd.bed_intervals(text), other_by_name.get(name, []))
        overlap_bed += overlap_contract.overlap_lines(text, per_row)
        summary += overlap_contract.summary_line(name, len(bases), totals)
    return overlap_bed, summary


def test_cli_simulated_record_against_its_truth(tmp_path):
    seq, truth = simulate_sequence(60_000, 23, 2, 30, lower_rate=0.2)
    fa, other, bed, obed, summary = (tmp_path / n for n in ("in.fa", "truth.bed", "out.bed", "overlap.bed", "summary.tsv"))
    write_fasta(str(fa), [("sim description dropped", seq)])
    other.write_text(truth_bed_text("sim", truth))
    r = _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--overlap-with", other, "--overlap-bed", obed, "--overlap-summary", summary, "--timing", tmp_path / "t.json"])
    assert "--overlap-with" not in r.stderr
    rows = bed.read_text()
    assert len(rows.splitlines()) > 10
    assert "".join(l.rsplit("\t", 2)[0] + "\n" for l in obed.read_text().splitlines()) == rows
    want_bed, want_summary = _expected(fa, rows, {"sim": [t[:2] for t in truth]})
    assert obed.read_text() == want_bed
    assert summary.read_text() == want_summary
    name, length, n_rows, rows_hit, n_other, other_hit, rows_bases, other_bases, both = summary.read_text().split("\t")
    assert (name, int(length), int(n_rows), int(n_other)) == ("sim", 60_000, len(rows.splitlines()), len(truth))
    assert int(other_hit) > len(truth) // 2 and 0 < int(both) <= min(int(rows_bases), int(other_bases))      # the tool finds its simulator's repeats
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "overlap" and stages.count("overlap") == 1
    # one of the two alone, and no key without them
    _run(["-i", fa, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--overlap-with", other, "--overlap-summary", tmp_path / "s.tsv", "--loci-bed", tmp_path / "l.bed",
          "--timing", tmp_path / "t2.json"])
    assert (tmp_path / "s.tsv").read_text() == want_summary
    assert list(_stages(tmp_path / "t2.json"))[-2:] == ["loci", "overlap"]
    _run(["-i", fa, "-o", tmp_path / "c.bed", "-m", 2, "-M", 30, "--timing", tmp_path / "t3.json"])
    assert "overlap" not in _stages(tmp_path / "t3.json")


def test_cli_two_records_and_an_unknown_name(tmp_path):
    recs = [("first", simulate_sequence(30_000, 31, 2, 30)), ("second", simulate_sequence(25_000, 32, 2, 30, lower_rate=0.3))]
    fa, other, bed, obed, summary = (tmp_path / n for n in ("in.fa", "other.bed", "out.bed", "overlap.bed", "summary.tsv"))
    write_fasta(str(fa), [(name, seq) for name, (seq, _) in recs])
    # OTHER: the truth of both records shifted by five bases, their lines interleaved, three lines of a name that is no record
    lines, by_name = ["# two records and a stranger\n"], {}
    for k in range(max(len(truth) for _, (_, truth) in recs)):
        for name, (_, truth) in reversed(recs):
            if k < len(truth):
                s, e = truth[k][0] + 5, truth[k][1] + 5
                lines.append(f"{name}\t{s}\t{e}\textra\n")
                by_name.setdefault(name, []).append((s, e))
        if k < 3:
            lines.append(f"stranger\t{k}\t{k + 10}\n")
    other.write_text("".join(lines))
    common = ["-i", fa, "-m", 2, "-M", 30, "--overlap-with", other]
    r = _run(common + ["-o", bed, "--overlap-bed", obed, "--overlap-summary", summary])
    assert r.stderr.endswith("ribbit-hip: --overlap-with: 3 intervals of 1 names that are no record of the input were ignored\n")
    assert r.stderr.count("--overlap-with") == 1
    want_bed, want_summary = _expected(fa, bed.read_text(), by_name)
    assert obed.read_text() == want_bed
    assert summary.read_text() == want_summary
    assert [l.split("\t")[0] for l in want_summary.splitlines()] == ["first", "second"]
    assert all(int(l.split("\t")[5]) > 0 for l in want_summary.splitlines())
    # two records in flight
    bed2, obed2, summary2 = (tmp_path / n for n in ("out2.bed", "overlap2.bed", "summary2.tsv"))
    _run(common + ["-o", bed2, "--overlap-bed", obed2, "--overlap-summary", summary2, "--jobs", 2])
    assert (bed2.read_text(), obed2.read_text(), summary2.read_text()) == (bed.read_text(), want_bed, want_summary)
