"""The rows by canonical motif class on the GPU (classes.hip through ribbit_hip_record_classes): Scanner.record_classes against the
host twin and the plain-Python statement of the contract (tests/classes_contract.py), and ribbit-hip --class-bed / --motif-summary
end to end."""
import numpy as np
import pytest

import classes_contract as cc
import ribbit_amd
import segments
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records

pytestmark = pytest.mark.gpu
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)      # the wave and block edges of the lane-per-row kernels
LONG_ROWS = (0, 1, 63, 64, 65)                   # how many rows of a call go through the long-motif kernel (and all of them)


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _pool(motifs):
    off = np.concatenate([[0], np.cumsum([len(m) for m in motifs], dtype=np.int64)]).astype(np.int32)
    return "".join(motifs).encode(), off


def _same(sc, length, iv, motifs, contract=True):
    """device == host twin (== contract); -> (classes per row, strands per row, groups as the contract has them)"""
    pool, off = _pool(motifs)
    classes, strands, groups = sc.record_classes(iv, pool, off)
    host = ribbit_amd.host_record_classes(length, iv, pool, off)
    assert (classes, strands) == host[:2], length
    assert groups.dtype == ribbit_amd.MOTIF_CLASS_DT and np.array_equal(groups, host[2]), length
    per_row = [classes[off[i]:off[i + 1]].decode() for i in range(len(motifs))]
    got = (per_row, list(strands.decode()),
           [(per_row[g["first_row"]], int(g["length"]), int(g["rows"]), int(g["bases"]), int(g["first_row"]), int(g["longest_row"])) for g in groups])
    if contract:
        assert got == cc.record_classes(length, iv, motifs), length
    return got


def _rows(n, length, seed):
    rs = np.random.RandomState(seed)
    starts = rs.randint(-20, length + 20, n)
    return np.stack([starts, starts + rs.randint(-5, 200, n)], 1)


def test_edge_sets_and_row_counts():
    rs = np.random.RandomState(1)
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in (0, 1, 64, 300, 4100):
            sc.load_record(_seq(length, length + 1))
            for iv, motifs in cc.edge_case_sets(length):
                cc.check_properties(length, iv, motifs, *_same(sc, length, iv, motifs))
        length = 4100
        for n in ROW_COUNTS:
            units = [cc.random_motif(rs, int(k)) for k in rs.randint(1, 33, 7)]
            motifs = [units[i % 7][i % len(units[i % 7]):] + units[i % 7][:i % len(units[i % 7])] for i in range(n)]
            got = _same(sc, length, _rows(n, length, n), motifs)
            cc.check_properties(length, _rows(n, length, n), motifs, *got)
            # all rows of one class: one group; all rows of distinct classes: n groups
            one = [("AC", "CA", "GT", "TG")[i % 4] for i in range(n)]
            assert [g[:3] for g in _same(sc, length, _rows(n, length, n + 1), one)[2]] == [("AC", 2, n)]
            distinct = ["A" * 6 + "".join("ACGT"[(i >> s) & 3] for s in (0, 2, 4, 6, 8)) + "C" for i in range(n)]
            assert len(_same(sc, length, _rows(n, length, n + 2), distinct)[2]) == n


def test_motif_lengths_and_the_long_row_compaction():
    rs = np.random.RandomState(2)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(5000, 3))
        for k in cc.MOTIF_LENGTHS:
            motifs = [cc.random_motif(rs, k) for _ in range(6)] + [cc.random_motif(rs, k, "AC") for _ in range(3)] + [cc.periodic("GTC", k)]
            motifs += [cc.reverse_complement(u[k // 3:] + u[:k // 3]) for u in motifs[:4]]
            got = _same(sc, 5000, _rows(len(motifs), 5000, k), motifs)
            cc.check_properties(5000, _rows(len(motifs), 5000, k), motifs, *got)
        # mixed in one call: so many rows of more than 32 bases among short ones, at scattered places; then all of them
        long_units = [cc.random_motif(rs, int(k)) for k in (33, 34, 63, 64, 65, 127, 200, 990)]
        for n_long in LONG_ROWS:
            n = 200
            where = set(rs.permutation(n)[:n_long].tolist())
            motifs = [long_units[i % 8] if i in where else cc.random_motif(rs, 1 + i % 32, "AC") for i in range(n)]
            cc.check_properties(5000, _rows(n, 5000, 5), motifs, *_same(sc, 5000, _rows(n, 5000, 5), motifs))
        motifs = [long_units[i % 8][i % 33:] + long_units[i % 8][:i % 33] for i in range(70)]
        assert len(_same(sc, 5000, _rows(70, 5000, 6), motifs)[2]) == 8
        # equal in their first 27 bases, different at base 28 and at the last one: the key alone cannot part these
        for k in (28, 33, 64, 500, 1023):
            twins = cc.key_twins(rs, k)
            twins += [cc.reverse_complement(u[5:] + u[:5]) for u in twins]
            got = _same(sc, 5000, _rows(8, 5000, 7), twins)
            assert got[0][:4] == twins[:4] and got[0][4:] == twins[:4] and got[1] == ["+"] * 4 + ["-"] * 4
            assert sorted(g[2] for g in got[2]) == ([2, 2, 4] if k > 28 else [4, 4])


def test_pool_offsets_of_every_alignment():
    """rows of 1 .. 17 bases, cycled: the motifs start at every offset mod 16 (the lanes read them in aligned 8-byte words)"""
    rs = np.random.RandomState(4)
    motifs = [cc.random_motif(rs, 1 + i % 17) for i in range(17 * 16 * 2)]
    _, off = _pool(motifs)
    assert {(int(o) % 16, int(k)) for o, k in zip(off[:-1], np.diff(off))} >= {(a, k) for a in range(16) for k in (1, 8, 16, 17)}
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(3000))
        cc.check_properties(3000, _rows(len(motifs), 3000, 1), motifs, *_same(sc, 3000, _rows(len(motifs), 3000, 1), motifs))
        # the same behind a lead of 1 .. 15 bases, with motifs of up to 32: every shift of the five-word window
        for lead in range(1, 16):
            shifted = ["A" * lead] + [cc.random_motif(rs, int(k)) for k in (32, 31, 25, 32, 24, 9, 32)]
            _same(sc, 3000, _rows(len(shifted), 3000, lead), shifted)


def test_many_rows_take_a_second_turn():
    """more rows of short motifs than one launch has lanes (1024 blocks of 256): compared with the host twin only"""
    n = 1024 * 256 + 65
    rs = np.random.RandomState(6)
    units = [cc.random_motif(rs, int(k)) for k in rs.randint(1, 13, 300)]
    motifs = [units[i] for i in rs.randint(0, len(units), n)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(100_000))
        classes, strands, groups = _same(sc, 100_000, _rows(n, 100_000, 8), motifs, contract=False)
        assert sum(g[2] for g in groups) == n and len(groups) == len({cc.motif_class(u)[0] for u in units})
        assert all(cc.motif_class(motifs[i]) == (classes[i], strands[i]) for i in range(0, n, 997))


def test_several_long_periodic_rows():
    """300 rows, each a periodic 1023-mer in which every comparison of tied rotations runs the full length"""
    units = ["ACG", "TCG", "AC", "AAT", "GATA", "T"]
    motifs = [cc.periodic(units[i % 6], 1023)[i % 7:] + cc.periodic(units[i % 6], 1023)[:i % 7] for i in range(300)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(5000))
        classes, strands, groups = _same(sc, 5000, _rows(300, 5000, 9), motifs, contract=False)
        want = {u: cc.motif_class(u) for u in set(motifs)}
        assert [(c, s) for c, s in zip(classes, strands)] == [want[u] for u in motifs]
        assert sum(g[2] for g in groups) == 300 and len(groups) == len({c for c, _ in want.values()})


def test_the_same_handle_twice_and_a_new_record():
    """nothing of a call shows through in the next: few rows after many, no rows, a record of length 0, back to the first"""
    rs = np.random.RandomState(9)
    units = [cc.random_motif(rs, int(k)) for k in (2, 3, 3, 5, 12, 31, 40, 200)]
    motifs = [units[i] for i in rs.randint(0, 8, 3000)]
    many = _rows(3000, 30_000, 10)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(30_000))
        first = _same(sc, 30_000, many, motifs)
        _same(sc, 30_000, many[:70], motifs[:70])
        _same(sc, 30_000, [(5, 9)], ["GT"])
        assert _same(sc, 30_000, [], []) == ([], [], [])
        assert _same(sc, 30_000, many, motifs) == first
        sc.load_record(_seq(9_000, 1))
        assert _same(sc, 9_000, many, motifs)[2] != first[2]
        sc.load_record(_seq(0))
        empty = _same(sc, 0, many, motifs)
        assert empty[:2] == first[:2] and len(empty[2]) == len(first[2]) and all(g[3] == 0 for g in empty[2])
        sc.load_record(_seq(30_000))
        assert _same(sc, 30_000, many, motifs) == first


def test_before_load_and_bad_arguments():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_classes([(0, 1)], ["AC"])
        sc.load_record(_seq(100))
        for motifs in (["AC", ""], ["ACN"], ["A" * 1024]):
            with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
                sc.record_classes([(0, 1)] * len(motifs), motifs)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            sc.record_classes([(0, 1), (0, 1)], b"ACGT", [0, 3, 2])
        assert _same(sc, 100, [(0, 1)], ["A" * 1023])[0] == ["A" * 1023]


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    length = len(seq)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        bed = sc.refine_bed("chr")
        rows = ribbit_amd.bed_intervals(bed)
        pool, off = ribbit_amd.bed_motifs(bed)
        assert len(rows) > 50_000 and len(off) == len(rows) + 1
        classes, strands, groups = sc.record_classes(rows, pool, off)
        host = ribbit_amd.host_record_classes(length, rows, pool, off)
        assert (classes, strands) == host[:2] and np.array_equal(groups, host[2])
        assert int(groups["rows"].sum()) == len(rows) and 1 < len(groups) < len(rows)
        width = np.clip(np.minimum(rows[:, 1].astype(np.int64), length) - np.maximum(rows[:, 0], 0), 0, None)
        assert int(groups["bases"].sum()) == int(width.sum())
        # every class line's longest row has that class
        for g in groups:
            a, b = (classes[off[i]:off[i + 1]] for i in (g["first_row"], g["longest_row"]))
            assert a == b and len(a) == g["length"]
        keys = [(int(g["length"]), classes[off[g["first_row"]]:off[g["first_row"] + 1]]) for g in groups]
        assert all(x < y for x, y in zip(keys, keys[1:]))
        for i in range(0, len(rows), 499):
            assert cc.motif_class(pool[off[i]:off[i + 1]].decode()) == (classes[off[i]:off[i + 1]].decode(), chr(strands[i]))


# ---- end to end
def _other_bed(fa, path):
    path.write_text("".join(f"{name}\t{k * 997}\t{k * 997 + 400}\n" for name, bases in records(fa) if name for k in range(len(bases) // 2000)))


def _expected(fa, bed):
    """the two files: per record, in input order, what the two text functions make of the host twin's classes of the record's BED rows"""
    by_name = rows_by_record(bed)
    class_bed, summary = b"", b""
    for name, bases in records(fa):
        rows = by_name.get(name, "")
        iv = ribbit_amd.bed_intervals(rows)
        pool, off = ribbit_amd.bed_motifs(rows)
        classes, strands, groups = ribbit_amd.host_record_classes(len(bases), iv, pool, off)
        class_bed += ribbit_amd.bed_class_text(rows, classes, off, strands)
        summary += ribbit_amd.class_summary_text(name, iv, classes, off, groups)
    return class_bed.decode(), summary.decode()


def test_cli_class_bed_and_motif_summary(tmp_path):
    fa, other = tmp_path / "in.fa", tmp_path / "other.bed"
    write_nine_records(fa, 300, 77)
    _other_bed(fa, other)
    common = ["-i", fa, "-m", 2, "-M", 30]
    bed0 = tmp_path / "plain.bed"
    _run(common + ["-o", bed0, "--best-bed", tmp_path / "plain.best.bed", "--timing", tmp_path / "t0.json"])
    want_bed = bed0.read_text()
    assert "classes" not in _stages(tmp_path / "t0.json")
    want_classes, want_summary = _expected(fa, want_bed)
    assert len(want_classes.splitlines()) == len(want_bed.splitlines()) and 0 < len(want_summary.splitlines()) < len(want_bed.splitlines())
    assert all(line.startswith(row + "\t") and line.count("\t") == row.count("\t") + 2 for line, row in zip(want_classes.splitlines(), want_bed.splitlines()))
    assert sum(int(line.split("\t")[-4]) for line in want_summary.splitlines()) == len(want_bed.splitlines())
    earlier = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed"]
    runs = [[], ["--jobs", "3"], ["--devices", "0,0", "--jobs", "2"],
            ["--overlap-with", other] + [x for k, option in enumerate(earlier) for x in (option, tmp_path / f"other{k}")]]
    for k, extra in enumerate(runs):
        bed, cls, summary, timing = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.class.bed", tmp_path / f"r{k}.classes.tsv", tmp_path / f"t{k + 1}.json"
        _run(common + ["-o", bed, "--class-bed", cls, "--motif-summary", summary, "--timing", timing] + extra)
        assert bed.read_text() == want_bed
        assert cls.read_text() == want_classes, extra
        assert summary.read_text() == want_summary, extra
        names = list(_stages(timing))
        assert names[-1] == "classes" and names.count("classes") == 1
    assert list(_stages(tmp_path / "t4.json"))[6:] == ["mask", "repeats", "loci", "density", "overlap", "best", "classes"]
    assert (tmp_path / "other6").read_text() == (tmp_path / "plain.best.bed").read_text()
    # either option alone makes the same file
    _run(common + ["-o", tmp_path / "a.bed", "--motif-summary", tmp_path / "a.tsv", "--timing", tmp_path / "ta.json"])
    assert (tmp_path / "a.tsv").read_text() == want_summary and list(_stages(tmp_path / "ta.json"))[-1] == "classes"
