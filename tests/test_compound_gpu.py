"""The rows chained into compound loci on the GPU (compound.hip through ribbit_hip_record_compounds): Scanner.record_compounds
against the host twin and the plain-Python statement of the contract (tests/compound_contract.py), against the loci of the same
handle, and ribbit-hip --compound-bed end to end."""
import numpy as np
import pytest

import compound_contract
import ribbit_amd
import segments
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from compound_contract import GAPS, I32_MAX, I32_MIN, LENGTHS

pytestmark = pytest.mark.gpu
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)      # the wave and block edges of the lane-per-row kernels


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _same(sc, length, iv, labels, gap, contract=True):
    compounds, members = sc.record_compounds(iv, labels, gap)
    assert compounds.dtype == ribbit_amd.COMPOUND_DT and members.dtype == np.int32
    host, host_members = ribbit_amd.host_record_compounds(length, iv, labels, gap)
    assert compounds.tobytes() == host.tobytes() and members.tolist() == host_members.tolist(), (length, gap)
    if contract:
        assert (compound_contract.as_dicts(compounds), members.tolist()) == compound_contract.record_compounds(length, iv, labels, gap), (length, gap)
    return compounds, members


def test_edge_sets_at_every_length_and_gap():
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in LENGTHS:
            sc.load_record(_seq(length, length + 1))
            for iv, labels in compound_contract.edge_case_sets(length):
                for gap in GAPS:
                    compounds, members = _same(sc, length, iv, labels, gap)
                    compound_contract.check_properties(length, iv, labels, compounds, members)


def test_row_counts_at_the_wave_and_block_edges():
    """rows of 5 bases every 15: at gap 9 every row is its own chain, at gap 10 all are one; with every other row empty the rest
    lie 25 apart"""
    length = 4100
    rs = np.random.RandomState(5)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(length, 3))
        for n in ROW_COUNTS:
            full = np.stack([15 * np.arange(n), 15 * np.arange(n) + 5], 1)
            holes = full.copy()
            holes[1::2] = holes[1::2, ::-1]
            perm = rs.permutation(n)
            for iv, apart, kept in ((full, 10, n), (holes, 25, (n + 1) // 2), (full[perm], 10, n)):
                for labels in (np.full(n, -7), np.arange(n) - n // 2, np.arange(n) % 3):
                    distinct = len(set(labels[:: 2 if iv is holes else 1].tolist()))
                    if iv is not full and iv is not holes:
                        labels = labels[perm]      # (a row's label goes where the row goes)
                    own, members = _same(sc, length, iv, labels, apart - 1)
                    assert len(own) == len(members) == kept and (own["rows"] == 1).all() and (own["classes"] == 1).all()
                    one, members = _same(sc, length, iv, labels, apart)
                    assert len(one) == 1 and len(members) == kept
                    assert (one["rows"][0], one["classes"][0], one["overlaps"][0], one["bases"][0]) == (kept, distinct, 0, 5 * kept)
                    assert one["switches"][0] == (0 if distinct == 1 else kept - 1)
                    compound_contract.check_properties(length, iv, labels, one, members)
                    _same(sc, length, iv, labels, I32_MAX)


def test_random_records():
    rs = np.random.RandomState(41)
    with ribbit_amd.Scanner(2, 30) as sc:
        for t in range(40):
            length, iv, labels = compound_contract.random_record(rs, t, (1, 3, 50)[t % 3])
            sc.load_record(_seq(length, t))
            for gap in GAPS:
                compounds, members = _same(sc, length, iv, labels, gap)
                compound_contract.check_properties(length, iv, labels, compounds, members)


def test_duplicates_keep_their_index_order_whatever_the_order():
    rows = [(100, 130)] * 4 + [(90, 120)] * 3 + [(100, 125), (100, 131), (300, 310), (300, 310)]
    labels = np.array([3, 1, 3, 2, 0, 0, 9, 4, 4, I32_MIN, I32_MAX])
    rs = np.random.RandomState(3)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(400, 1))
        compounds, members = _same(sc, 400, rows, labels, 7)
        assert members.tolist() == [4, 5, 6, 7, 0, 1, 2, 3, 8, 9, 10]
        assert compound_contract.as_dicts(compounds) == [dict(bases=266, start=90, end=131, rows=9, classes=6, switches=7, overlaps=8, first=0, pad=0),
                                                         dict(bases=20, start=300, end=310, rows=2, classes=2, switches=1, overlaps=1, first=9, pad=0)]
        for _ in range(20):
            perm = rs.permutation(len(rows))
            shuffled = [rows[i] for i in perm]
            got, got_members = _same(sc, 400, shuffled, labels[perm], 7)
            assert [shuffled[i] for i in got_members] == [rows[i] for i in members]
            for row in set(rows):      # among identical rows the indices ascend
                same = [i for i in got_members.tolist() if shuffled[i] == row]
                assert same == sorted(same)
            assert all(np.array_equal(got[f], compounds[f]) for f in ("start", "end", "rows", "bases", "classes", "overlaps", "first"))


def test_chains_are_the_loci_of_the_same_handle():
    rs = np.random.RandomState(9)
    starts = rs.randint(-50, 30_050, 3000)
    iv = np.stack([starts, starts + rs.randint(-5, 60, 3000)], 1)
    labels = rs.randint(0, 4, 3000)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(30_000))
        for gap in (0, 5, 1000):
            compounds, _ = _same(sc, 30_000, iv, labels, gap)
            loci = sc.record_loci(iv, gap)
            assert len(loci) >= (1 if gap == 1000 else 100) and all(np.array_equal(compounds[f], loci[f]) for f in ("start", "end", "rows")), gap
            # the loci call has used the handle in between
            again, _ = _same(sc, 30_000, iv, labels, gap)
            assert again.tobytes() == compounds.tobytes()


def test_one_chain_of_many_rows():
    """every row overlaps the next; a chain of every row costs no more than a chain of one"""
    n = 20_000
    length = 10 * (n - 1) + 15 + 10
    chain = np.stack([10 * np.arange(n), 10 * np.arange(n) + 15], 1)
    labels = np.arange(n) % 7 - 3
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(b"ACGT" * (length // 4) + b"A" * (length % 4))
        one, members = _same(sc, length, chain, labels, 0)
        assert compound_contract.as_dicts(one) == [dict(bases=15 * n, start=0, end=10 * (n - 1) + 15, rows=n, classes=7, switches=n - 1, overlaps=n - 1, first=0, pad=0)]
        assert members.tolist() == list(range(n))
        perm = np.random.RandomState(2).permutation(n)
        got, got_members = _same(sc, length, chain[perm], labels[perm], 0)
        assert got.tobytes() == one.tobytes() and perm[got_members].tolist() == list(range(n))


def test_many_chains_and_more_rows_than_lanes():
    """every sorted position is a head: disjoint rows at gap 0; then more rows than one launch has lanes (1024 blocks of 256), short
    ones, some empty or out of range: the lanes of the first blocks take a second turn"""
    n = 100_000
    rows = np.stack([10 * np.arange(n), 10 * np.arange(n) + 5], 1)
    labels = np.arange(n) % 5
    perm = np.random.RandomState(4).permutation(n)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(b"ACGT" * (10 * n // 4))
        own, members = _same(sc, 10 * n, rows, labels, 0, contract=False)
        assert len(own) == n and members.tolist() == list(range(n))
        assert np.array_equal(own["start"], rows[:, 0]) and np.array_equal(own["end"], rows[:, 1]) and np.array_equal(own["first"], np.arange(n))
        assert (own["rows"] == 1).all() and (own["classes"] == 1).all() and (own["bases"] == 5).all() and (own["switches"] == 0).all()
        got, got_members = _same(sc, 10 * n, rows[perm], labels[perm], 0, contract=False)
        assert got.tobytes() == own.tobytes() and perm[got_members].tolist() == list(range(n))
        rs = np.random.RandomState(17)
        starts = rs.randint(-20, 10 * n + 20, 1024 * 256 + 65)
        wide = np.stack([starts, starts + rs.randint(-3, 40, len(starts))], 1)
        wide_labels = rs.randint(I32_MIN, I32_MAX, len(starts), dtype=np.int64) % 11 - 5
        for gap in (0, 3):
            compounds, members = _same(sc, 10 * n, wide, wide_labels, gap, contract=False)
            compound_contract.check_properties(10 * n, wide, wide_labels, compounds, members)
            assert 100 < len(compounds) < len(members) < len(wide)      # (a few thousand chains at gap 0, about a thousand at gap 3)


def test_the_same_handle_twice_and_a_new_record():
    """nothing of a call shows through in the next: fewer rows after many, other rows of the same number, a shorter record"""
    rs = np.random.RandomState(9)
    starts = rs.randint(-50, 30_050, 3000)
    many = np.stack([starts, starts + rs.randint(-5, 400, 3000)], 1)
    labels = rs.randint(-2, 3, 3000)

    def both(sc, length, iv, lab, gap=100):
        compounds, members = _same(sc, length, iv, lab, gap)
        return compounds.tobytes(), members.tolist()

    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(30_000))
        first = both(sc, 30_000, many, labels)
        both(sc, 30_000, many[:70], labels[:70])
        both(sc, 30_000, many[::-1], labels[::-1])
        both(sc, 30_000, [(5, 9)], [1])
        assert both(sc, 30_000, [], []) == (b"", [])
        assert both(sc, 30_000, [(9, 5), (40_000, 50_000)], [1, 2]) == (b"", [])
        assert both(sc, 30_000, many, labels) == first
        assert both(sc, 30_000, many[:70], labels[:70], 0) != both(sc, 30_000, many[:70], labels[:70])
        sc.load_record(_seq(9_000, 1))
        assert both(sc, 9_000, many, labels) != first
        sc.load_record(_seq(0))
        assert both(sc, 0, many, labels) == (b"", [])
        sc.load_record(_seq(30_000))
        assert both(sc, 30_000, many, labels) == first
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: gap -1 is negative"):
            sc.record_compounds(many, labels, -1)


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_compounds([(0, 1)], [0])


def _kinds(compounds):
    return {"p": int((compounds["rows"] == 1).sum()), "i": int(((compounds["rows"] > 1) & (compounds["classes"] == 1)).sum()),
            "c": int((compounds["classes"] > 1).sum())}


def test_two_megabase_record_with_its_bed_rows():
    """best rows, then classes, then labels, then compounds, all on one handle; the simulated record of seed 500 has chains of
    every kind"""
    seq = segments.simulated_record(2_000_000, 500)
    length = len(seq)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        bed = sc.refine_bed("chr")
        rows = ribbit_amd.bed_intervals(bed)
        chosen, _ = sc.record_best(rows)
        assert 1000 < len(chosen) < len(rows)
        lines = ribbit_amd.bed_rows_text(bed, chosen)
        motifs, offsets = ribbit_amd.bed_motifs(lines)
        iv = rows[chosen]
        classes, _, groups = sc.record_classes(iv, motifs, offsets)
        labels = ribbit_amd.class_labels(classes, offsets, groups)
        assert labels.max() == len(groups) - 1 and len(np.unique(labels)) == len(groups)
        compounds, members = _same(sc, length, iv, labels, 100, contract=False)
        compound_contract.check_properties(length, iv, labels, compounds, members)
        assert members.tolist() == list(range(len(iv)))      # (the selection comes by ascending start)
        assert (compounds["overlaps"] == 0).all()
        kinds = _kinds(compounds)
        print("chains by kind:", kinds)
        assert min(kinds.values()) >= 1, kinds
        loci = sc.record_loci(iv, 100)
        assert all(np.array_equal(compounds[f], loci[f]) for f in ("start", "end", "rows")) and np.array_equal(compounds["bases"], loci["covered"])
        text = ribbit_amd.compound_text("chr", lines, length, iv, compounds, members).decode().splitlines()
        assert len(text) == len(compounds) and {line.split("\t")[3] for line in text} == {"p", "i", "c"}


# ---- end to end
def _other_bed(fa, path):
    path.write_text("".join(f"{name}\t{k * 997}\t{k * 997 + 400}\n" for name, bases in records(fa) if name for k in range(len(bases) // 2000)))


def _expected(fa, bed, gap):
    """the file: per record, in input order, what the host twins make of the record's BED rows"""
    by_name = rows_by_record(bed)
    text = b""
    for name, bases in records(fa):
        rows = by_name.get(name, "")
        chosen, _ = ribbit_amd.host_record_best(len(bases), ribbit_amd.bed_intervals(rows))
        lines = ribbit_amd.bed_rows_text(rows, chosen)
        motifs, offsets = ribbit_amd.bed_motifs(lines)
        iv = ribbit_amd.bed_intervals(lines)
        classes, _, groups = ribbit_amd.host_record_classes(len(bases), iv, motifs, offsets)
        labels = ribbit_amd.class_labels(classes, offsets, groups)
        compounds, members = ribbit_amd.host_record_compounds(len(bases), iv, labels, gap)
        text += ribbit_amd.compound_text(name, lines, len(bases), iv, compounds, members)
    return text.decode()


def test_cli_compound_bed(tmp_path):
    fa, other = tmp_path / "in.fa", tmp_path / "other.bed"
    write_nine_records(fa, 300, 77)
    _other_bed(fa, other)
    common = ["-i", fa, "-m", 2, "-M", 30]
    bed0, best0 = tmp_path / "plain.bed", tmp_path / "plain.best.bed"
    _run(common + ["-o", bed0, "--best-bed", best0, "--timing", tmp_path / "t0.json"])
    want_bed, want_best = bed0.read_text(), best0.read_text()
    assert "compound" not in _stages(tmp_path / "t0.json")
    want = _expected(fa, want_bed, 100)
    kinds = [line.split("\t")[3] for line in want.splitlines()]
    assert 0 < len(kinds) <= len(want_best.splitlines()) and set(kinds) <= {"p", "i", "c"} and "p" in kinds
    nine = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--class-bed", "--motif-summary"]
    runs = [[], ["--jobs", "3"], ["--devices", "0,0", "--jobs", "2"],
            ["--overlap-with", other] + [x for k, option in enumerate(nine) for x in (option, tmp_path / f"other{k}")]]
    for k, extra in enumerate(runs):
        bed, best, compound, timing = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.best.bed", tmp_path / f"r{k}.compound.bed", tmp_path / f"t{k + 1}.json"
        _run(common + ["-o", bed, "--best-bed", best, "--compound-bed", compound, "--timing", timing] + extra)
        assert bed.read_text() == want_bed
        assert best.read_text() == want_best
        assert compound.read_text() == want, extra
        assert list(_stages(timing))[-1] == "compound"
    assert list(_stages(tmp_path / "t4.json"))[6:] == ["mask", "repeats", "loci", "density", "overlap", "best", "classes", "compound"]
    # without --best-bed beside it, and at another gap
    alone, apart = tmp_path / "alone.compound.bed", tmp_path / "apart.compound.bed"
    _run(common + ["-o", tmp_path / "alone.bed", "--compound-bed", alone, "--timing", tmp_path / "t5.json"])
    assert alone.read_text() == want and (tmp_path / "alone.bed").read_text() == want_bed
    assert list(_stages(tmp_path / "t5.json"))[6:] == ["compound"]
    _run(common + ["-o", tmp_path / "apart.bed", "--compound-bed", apart, "--compound-gap", "0"])
    assert apart.read_text() == _expected(fa, want_bed, 0) != want
