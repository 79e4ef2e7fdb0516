"""The nearest target of every query on the GPU (nearest.hip through ribbit_hip_record_nearest): Scanner.record_nearest
against the host twin and the plain statement of the contract (tests/nearest_contract.py), and ribbit-hip --overlap-with /
--nearest-bed / --nearest-other-bed end to end."""
import numpy as np
import pytest

import nearest_contract as nc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages
from ribbit_amd.simulate import simulate_sequence, truth_bed_text, write_fasta

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 64, 1000)
# a launch has at most 1024 blocks of 256 lanes (nearest.hip): beyond that the key kernel and the query kernel stride
STRIDE_LANES = 1024 * 256


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _same(sc, length, queries, targets, what=None):
    """the device equals the twin and the contract"""
    got = sc.record_nearest(queries, targets)
    assert got.dtype == ribbit_amd.NEAREST_DT and got.shape == (len(queries),)
    assert got.tolist() == ribbit_amd.host_record_nearest(length, queries, targets).tolist(), (length, what)
    assert nc.as_tuples(got) == nc.record_nearest(length, queries, targets), (length, what)
    return got


@pytest.mark.parametrize("length", LENGTHS)
def test_edge_case_sets(length):
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length, length))
        for what, queries, targets in nc.edge_case_sets(length):
            _same(sc, length, queries, targets, what)
            _same(sc, length, targets, queries, what)


def test_random_sets():
    length = 100_000
    rs = np.random.RandomState(92)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length))
        for t in range(12):
            queries, targets = nc.random_sets(length, rs, int(rs.randint(0, 300)), int(rs.randint(0, 300)), 60 if t % 2 else 4000, reach=50)
            _same(sc, length, queries, targets, t)


def test_small_target_counts():
    """no target, one and two, empty ones among them: the empty targets' keys and the bounds of the four searches"""
    length = 200
    rs = np.random.RandomState(3)
    queries = [(0, 1), (0, length), (length - 1, length), (50, 60), (60, 70), (40, 50), (55, 56), (49, 61), (-3, 0), (70, 60)] + nc.random_sets(length, rs, 90, 0, 30)[0].tolist()
    one = [[(50, 60)], [(0, 1)], [(length - 1, length)], [(0, length)], [(-5, length + 5)], [(60, 50)], [(length, length + 3)]]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length))
        _same(sc, length, queries, [], "no target")
        for a in one:
            _same(sc, length, queries, a, a)
            for b in one:
                _same(sc, length, queries, a + b, (a, b))


def test_sizes_beyond_one_stride():
    """more queries and more targets than one launch has lanes: both one-lane-per-item kernels stride"""
    rs = np.random.RandomState(18)
    length, many = 1_000_000, 300_000
    assert many > STRIDE_LANES
    def one():
        starts = rs.randint(-20, length + 20, many)
        return np.stack([starts, starts + rs.randint(-3, 40, many)], 1)
    queries, targets = one(), one()
    targets[::3000, 1] += 5_000          # (some long ones: containers)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(b"ACGT" * (length // 4))
        got = sc.record_nearest(queries, targets)
    assert got.tolist() == ribbit_amd.host_record_nearest(length, queries, targets).tolist()
    want = nc.record_nearest_without_loops(length, queries, targets)
    assert np.array_equal(nc.as_array(got), want)
    assert [int((want[:, 0] == k).sum()) > 1000 for k in (nc.APART, nc.OVER, nc.INSIDE)] == [True] * 3


def test_second_call_and_new_record():
    """the same arguments again, other sets, and another record on the same handle: what an earlier call handed out is not relied on"""
    rs = np.random.RandomState(6)
    queries, targets = nc.random_sets(20_000, rs, 200, 150, 700, reach=50)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(20_000))
        first = _same(sc, 20_000, queries, targets)
        assert _same(sc, 20_000, queries, targets).tolist() == first.tolist()
        _same(sc, 20_000, queries[:90], targets[:70])
        _same(sc, 20_000, targets, queries)
        sc.load_record(_seq(9_000, 1))
        shorter = _same(sc, 9_000, queries, targets)
        assert shorter.tolist() != first.tolist()
        sc.load_record(_seq(0))
        _same(sc, 0, queries, targets)
        sc.load_record(_seq(20_000))
        assert _same(sc, 20_000, queries, targets).tolist() == first.tolist()


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_nearest([(0, 1)], [(0, 1)])


def test_between_the_other_row_outputs():
    """the best rows, the classes and the overlap in between, on one handle: they share the staging buffers and the scratch"""
    rs = np.random.RandomState(7)
    length = 30_000
    queries, targets = nc.random_sets(length, rs, 400, 300, 500, reach=50)
    motifs = ["ACGTAG"[:1 + k % 6] for k in range(len(queries))]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length))
        best = sc.record_best(queries)
        first = _same(sc, length, queries, targets)
        classes = sc.record_classes(queries, motifs)
        assert _same(sc, length, targets, queries).shape == (len(targets),)
        overlap = sc.record_overlap(queries, targets)
        assert _same(sc, length, queries, targets).tolist() == first.tolist()
        again = sc.record_best(queries)
        assert again[0].tolist() == best[0].tolist() and again[1] == best[1]
        assert sc.record_classes(queries, motifs)[0] == classes[0]
        assert sc.record_overlap(queries, targets)[0].tolist() == overlap[0].tolist()
        assert ((first["kind"] > 0) == (overlap[0][:, 0] > 0)).all()


# ---- end to end
def _labelled(lines):
    """the intervals and labels of one record's lines of an other file, as the tool reads them"""
    iv, labels = [], []
    for line in lines:
        cols = line.rstrip("\n").split("\t")
        iv.append((int(cols[1]), int(cols[2])))
        labels.append(cols[3] if len(cols) > 3 and cols[3] else ".")
    return iv, labels


def _expected(fa, bed, other_lines_by_name):
    """the two files: the contract and the plain formatter applied to the BED and the other file's lines per record, in input order"""
    by_name = rows_by_record(bed)
    nearest_bed, other_bed = "", ""
    for name, bases in records(fa):
        text = by_name.get(name, "")
        rows = ribbit_amd.bed_intervals(text).tolist()
        iv, labels = _labelled(other_lines_by_name.get(name, []))
        nearest_bed += nc.nearest_lines(text, nc.record_nearest(len(bases), rows, iv), iv, labels)
        if iv:
            motifs = [line.split("\t")[3] for line in text.splitlines()]
            other_bed += nc.other_lines(name, iv, labels, nc.record_nearest(len(bases), iv, rows), rows, motifs)
    return nearest_bed, other_bed


def test_cli_simulated_record_against_its_truth(tmp_path):
    seq, truth = simulate_sequence(200_000, 24, 2, 30, lower_rate=0.2)
    fa, other, bed, nbed, obed, ovl = (tmp_path / n for n in ("in.fa", "truth.bed", "out.bed", "nearest.bed", "nearest_other.bed", "overlap.bed"))
    write_fasta(str(fa), [("sim description dropped", seq)])
    other.write_text(truth_bed_text("sim", truth))
    r = _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--overlap-with", other, "--nearest-bed", nbed, "--nearest-other-bed", obed, "--overlap-bed", ovl,
              "--timing", tmp_path / "t.json"])
    assert "--overlap-with" not in r.stderr
    rows = bed.read_text()
    assert len(rows.splitlines()) > 30
    got = nbed.read_text()
    assert "".join(l.rsplit("\t", 8)[0] + "\n" for l in got.splitlines()) == rows
    want_bed, want_other = _expected(fa, rows, {"sim": other.read_text().splitlines()})
    assert got == want_bed
    assert obed.read_text() == want_other
    assert len(want_other.splitlines()) == len(truth)
    # every row that is in or over an interval overlaps at least one, by --overlap-bed of the same run
    kinds = [l.split("\t")[11] for l in got.splitlines()]
    counts = [int(l.split("\t")[11]) for l in ovl.read_text().splitlines()]
    assert [k != "." for k in kinds] == [c > 0 for c in counts]
    assert kinds.count("in") + kinds.count("over") > len(kinds) // 2          # the tool finds its simulator's repeats
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "nearest" and stages.count("nearest") == 1
    # one of the two alone beside another output
    _run(["-i", fa, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--overlap-with", other, "--nearest-other-bed", tmp_path / "o.bed", "--loci-bed", tmp_path / "l.bed",
          "--timing", tmp_path / "t2.json"])
    assert (tmp_path / "o.bed").read_text() == want_other
    assert list(_stages(tmp_path / "t2.json"))[-2:] == ["loci", "nearest"]


def test_cli_two_records_and_an_unknown_name(tmp_path):
    recs = [("first", simulate_sequence(30_000, 31, 2, 30)), ("second", simulate_sequence(25_000, 32, 2, 30, lower_rate=0.3)),
            ("third", simulate_sequence(20_000, 33, 2, 30))]
    fa, other, bed, nbed, obed = (tmp_path / n for n in ("in.fa", "other.bed", "out.bed", "nearest.bed", "nearest_other.bed"))
    write_fasta(str(fa), [(name, seq) for name, (seq, _) in recs])
    # the other file: the truth of the first two records shifted by five bases, their lines interleaved, with a label, with an empty
    # label and without a fourth column in turn; three lines of a name that is no record; nothing for the third record
    lines, by_name = ["# two records and a stranger\n"], {}
    for k in range(max(len(truth) for _, (_, truth) in recs[:2])):
        for name, (_, truth) in reversed(recs[:2]):
            if k < len(truth):
                s, e = truth[k][0] + 5, truth[k][1] + 5
                line = f"{name}\t{s}\t{e}" + (f"\tlocus {k} of {name}\t0\t+", "\t\textra", "")[k % 3] + "\n"
                lines.append(line)
                by_name.setdefault(name, []).append(line)
        if k < 3:
            lines.append(f"stranger\t{k}\t{k + 10}\tunknown\n")
    other.write_text("".join(lines))
    common = ["-i", fa, "-m", 2, "-M", 30, "--overlap-with", other]
    r = _run(common + ["-o", bed, "--nearest-bed", nbed, "--nearest-other-bed", obed])
    assert r.stderr.endswith("ribbit-hip: --overlap-with: 3 intervals of 1 names that are no record of the input were ignored\n")
    assert r.stderr.count("--overlap-with") == 1
    want_bed, want_other = _expected(fa, bed.read_text(), by_name)
    assert nbed.read_text() == want_bed
    assert obed.read_text() == want_other
    # the order: the records' order, and within a record the file's; no line for the third record, whose rows have '.' throughout
    assert [l.split("\t")[:3] for l in want_other.splitlines()] == [l.rstrip("\n").split("\t")[:3] for name in ("first", "second") for l in by_name[name]]
    labels = {l.split("\t")[3] for l in want_other.splitlines()}
    assert "." in labels and "locus 0 of first" in labels and "stranger" not in want_other and "unknown" not in want_bed
    third = [l for l in want_bed.splitlines() if l.startswith("third\t")]
    assert third and all(l.endswith("\t." * 8) for l in third)
    # two records in flight
    bed2, nbed2, obed2 = (tmp_path / n for n in ("out2.bed", "nearest2.bed", "nearest_other2.bed"))
    _run(common + ["-o", bed2, "--nearest-bed", nbed2, "--nearest-other-bed", obed2, "--jobs", 2])
    assert (bed2.read_text(), nbed2.read_text(), obed2.read_text()) == (bed.read_text(), want_bed, want_other)
