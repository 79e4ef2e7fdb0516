"""The rows' CIGARs decoded on the GPU (interruptions.hip through ribbit_hip_record_interruptions): Scanner.record_interruptions
against the host twin and the plain-Python statement of the contract (tests/interruptions_contract.py), and ribbit-hip
--interruption-bed / --purity-bed end to end."""
import numpy as np
import pytest

import interruptions_contract as ic
import ribbit_amd
import segments
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records

pytestmark = pytest.mark.gpu
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257)      # the wave and block edges of the lane-per-row kernels


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgtn", np.uint8)[np.random.RandomState(seed).randint(0, 10, n)].tobytes()


def _same(sc, sequence, iv, ks, cigars, contract=True):
    """device == host twin (== contract); -> the result in the contract's form"""
    got = sc.record_interruptions(iv, ks, cigars)
    host = ribbit_amd.host_record_interruptions(sequence, iv, ks, cigars)
    assert got[0].dtype == ribbit_amd.ROW_PURITY_DT and got[1].dtype == ribbit_amd.INTERRUPTION_DT and got[3].dtype == np.int32
    for a, b, what in zip(got, host, ("rows", "sites", "observed", "offsets")):
        assert (a == b) if isinstance(a, bytes) else np.array_equal(a, b), what
    if not contract:
        return got
    result = ic.unpack(*got)
    assert result == ic.record_interruptions(sequence, iv, cigars)
    return result


def _rows(rs, n, length, cigars):
    starts = rs.randint(-20, length + 20, n)
    return np.stack([starts, starts + [ic.query_of(c) + (0 if rs.randint(5) else 1) for c in cigars]], 1)


def test_row_counts():
    rs = np.random.RandomState(1)
    seq = _seq(4100, 1)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        for n in ROW_COUNTS:
            cigars = [ic.random_cigar(rs, int(k)) for k in rs.randint(0, 9, n)]
            iv, ks = _rows(rs, n, len(seq), cigars), rs.randint(1, 9, n)
            ic.check_properties(seq, iv, cigars, *_same(sc, seq, iv, ks, cigars))
            # all rows without a CIGAR; all rows one match; all rows one interruption
            assert _same(sc, seq, iv, ks, [b""] * n)[1] == []
            assert _same(sc, seq, iv, ks, [b"5="] * n)[1] == []
            assert len(_same(sc, seq, iv, ks, [b"2X1I3D"] * n)[1]) == n


def test_cigar_shapes_and_clipping():
    """every shape of the contract at every clipping of a row: before 0, past L, wholly outside; N and lower case are kept"""
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in (0, 1, 64, 300, 4100):
            seq = _seq(length, length + 1)
            sc.load_record(seq)
            for iv, ks, cigars in ic.edge_case_sets(length):
                ic.check_properties(seq, iv, cigars, *_same(sc, seq, iv, ks, cigars))
        seq = b"ACGTNacgtnACGTACGTAC"
        sc.load_record(seq)
        one = lambda s, c: _same(sc, seq, [(s, s + ic.query_of(c))], [2], [c])
        assert one(3, b"") == ([(0, 0, 0, 0, 0, 0, 3, 3)], [], [])
        assert one(3, b"5=") == ([(0, 0, 0, 0, 0, 5, 3, 8)], [], [])
        assert one(1, b"2X5=1I") == ([(0, 2, 2, 1, 0, 8, 3, 8)], [(0, 1, 3, 2, 0, 0, 0, 2), (0, 8, 9, 0, 1, 0, 4, 2)], [b"CG", b"t"])
        assert one(4, b"2X1I3D") == ([(0, 1, 2, 1, 3, 3, 4, 4)], [(0, 4, 7, 2, 1, 3, 0, 6)], [b"Nac"])
        assert one(0, b"3=2M4=") == ([(0, 0, 0, 0, 0, 9, 0, 9)], [], [])
        assert one(2, b"3=1X3=1X2=")[0] == [(0, 2, 2, 0, 0, 10, 2, 5)]      # two equal longest stretches: the leftmost
        assert one(2, b"2=1X3=1X3=")[0] == [(0, 2, 2, 0, 0, 10, 5, 8)]
        assert one(5, b"2=3D2=") == ([(0, 1, 0, 0, 3, 4, 5, 7)], [(0, 7, 7, 0, 0, 3, 2, 2)], [b""])
        assert one(0, b"2147483647=")[0] == [(0, 0, 0, 0, 0, 2147483647, 0, 2147483647)]
        assert one(-5, b"0000000003X2=") == ([(0, 1, 3, 0, 0, 5, -2, 0)], [(0, -5, -2, 3, 0, 0, 0, 11)], [b""])


def test_pool_offsets_of_every_alignment():
    """CIGARs of 2 .. 17 bytes, cycled (no CIGAR has one byte: an op has a digit and a letter; a second one of 3 bytes makes the
    cycle's length odd): they start at every offset mod 16, and the lanes read the pool in aligned 16-byte pieces"""
    rs = np.random.RandomState(4)
    cycle = list(range(2, 18)) + [3]
    cigars = [ic.cigar_of_bytes(rs, cycle[i % 17]) for i in range(17 * 16 * 2)]
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigars])])
    assert {(int(o) % 16, int(k)) for o, k in zip(off[:-1], np.diff(off))} >= {(a, k) for a in range(16) for k in (2, 8, 16, 17)}
    seq = _seq(3000)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        iv, ks = _rows(rs, len(cigars), 3000, cigars), rs.randint(1, 9, len(cigars))
        ic.check_properties(seq, iv, cigars, *_same(sc, seq, iv, ks, cigars))
        # the same behind a lead of 2 .. 15 and 17 bytes (17: offset 1), with CIGARs that cross one and two 16-byte pieces
        for lead in list(range(2, 16)) + [17]:
            shifted = [ic.cigar_of_bytes(rs, lead)] + [ic.cigar_of_bytes(rs, int(k)) for k in (16, 15, 17, 32, 2, 33, 9, 31)]
            _same(sc, seq, _rows(rs, len(shifted), 3000, shifted), [3] * len(shifted), shifted)


def test_skewed_rows():
    """one row of 20,000 ops among 300 rows of one op, and one row whose single interruption has 9000 ops: in the middle of the
    rows, so that the long row starts inside one tile of the scans and ends tiles later"""
    rs = np.random.RandomState(5)
    seq = _seq(30_000, 5)
    small = [(b"7=", b"3X", b"2I", b"4D", b"9M")[i % 5] for i in range(300)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        for long_row, n_sites in ((b"1=1X" * 10_000, 10_000), (b"5=" + b"1X1I1D" * 3000 + b"5=", 1)):
            for where in (0, 150, 299):
                cigars = small[:where] + [long_row] + small[where:]
                iv, ks = _rows(rs, len(cigars), 10_000, cigars), rs.randint(1, 9, len(cigars))
                rows, sites, observed = _same(sc, seq, iv, ks, cigars)
                assert rows[where][1] == n_sites and rows[where][0] == sum(c[-1:] in b"XID" for c in small[:where])
            ic.check_properties(seq, iv, cigars, rows, sites, observed)


def test_many_rows_take_a_second_turn():
    """more rows than one launch has lanes (1024 blocks of 256): compared with the host twin only"""
    n = 1024 * 256 + 65
    rs = np.random.RandomState(6)
    shapes = [ic.random_cigar(rs, int(k)) for k in rs.randint(0, 7, 200)]
    spans = np.array([ic.query_of(c) for c in shapes])
    pick = rs.randint(0, 200, n)
    cigars = [shapes[i] for i in pick]
    starts = rs.randint(-20, 100_020, n)
    iv = np.stack([starts, starts + spans[pick]], 1)
    seq = _seq(100_000)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        rows, sites, observed, offsets = _same(sc, seq, iv, np.ones(n, dtype=np.int32), cigars, contract=False)
        assert len(rows) == n and int(rows["count"].sum()) == len(sites) and int(offsets[-1]) == len(observed)
        few = list(range(0, n, 9973))
        want = ic.record_interruptions(seq, iv[few], [cigars[i] for i in few])
        assert [tuple(int(rows[i][f]) for f in ic.ROW_FIELDS[1:]) for i in few] == [r[1:] for r in want[0]]


def test_the_same_handle_twice_and_a_new_record():
    """nothing of a call shows through in the next: few rows after many, no rows, a record of length 0, back to the first"""
    rs = np.random.RandomState(9)
    cigars = [ic.random_cigar(rs, int(k)) for k in rs.randint(0, 12, 3000)]
    many, ks = _rows(rs, 3000, 30_000, cigars), rs.randint(1, 9, 3000)
    seq = _seq(30_000)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        first = _same(sc, seq, many, ks, cigars)
        _same(sc, seq, many[:70], ks[:70], cigars[:70])
        _same(sc, seq, [(5, 9)], [2], [b"2=1X1="])
        assert _same(sc, seq, [], [], []) == ([], [], [])
        assert _same(sc, seq, many, ks, cigars) == first
        other = _seq(9_000, 1)
        sc.load_record(other)
        assert _same(sc, other, many, ks, cigars)[2] != first[2]
        sc.load_record(b"")
        empty = _same(sc, b"", many, ks, cigars)
        assert empty[:2] == first[:2] and all(o == b"" for o in empty[2])
        sc.load_record(seq)
        assert _same(sc, seq, many, ks, cigars) == first


def test_before_load_and_bad_grammar():
    L = ribbit_amd.load_library()
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_interruptions([(0, 1)], [2], [b"1="])
        seq = _seq(100)
        sc.load_record(seq)

        def refused(cigars, iv=None, ks=None, offsets=None):
            iv = [(0, 1)] * (len(cigars) if offsets is None else len(offsets) - 1) if iv is None else iv
            ks = [1] * len(iv) if ks is None else ks
            with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
                ribbit_amd.host_record_interruptions(seq, iv, ks, cigars, offsets)
            want = L.ribbit_hip_last_error().decode()
            with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
                sc.record_interruptions(iv, ks, cigars, offsets)
            assert L.ribbit_hip_last_error().decode() == want      # the device refuses what the twin refuses, in its words
            return want

        good = [b"3=1X3=1X5=1D82=", b"", b"16="]
        assert "byte 21 (row 3) is neither" in refused(good + [b"3=1Y2="])
        assert "byte 17 (row 2) is an op letter without" in refused(good[:2] + [b"1X=5"])
        assert "byte 29 (row 3) ends an op of more than ten digits" in refused(good + [b"12345678901="])
        assert "byte 35 (row 3) ends an op of more than ten digits" in refused(good + [b"00000000000000001="])
        assert "byte 19 (row 3) ends an op whose length is not" in refused(good + [b"0X"])
        assert "byte 28 (row 3) ends an op whose length is not" in refused(good + [b"2147483648="])
        assert "byte 20 (row 3) is the row's end" in refused(good + [b"12", b"3="])
        assert "byte 1 (row 0) is the row's end" in refused([b"7"])      # one byte is no CIGAR
        assert "row 1: the CIGAR's op lengths sum to 2147483648" in refused([b"5=", b"2147483647=1D"])
        assert "row 1: its start 1 and its CIGAR's query length 2147483647" in refused([b"1=", b"2147483647="], iv=[(0, 1), (1, 5)])
        assert "byte 14 (row 0) is neither" in refused([b"2147483647=1D1Y", b"=1"])
        # the lowest offending byte is the one named, whichever 16-byte piece it lies in
        for at in (0, 15, 16, 17, 31, 32, 100):
            pool = bytearray(b"1=" * 60)
            pool[at] = ord("y")
            pool[110] = ord("?")
            assert f"byte {at} (row {at // 40}) is neither" in refused([bytes(pool[k:k + 40]) for k in (0, 40, 80)])
        assert "a motif of 0 bases" in refused([b"5="], ks=[0])
        assert "do not ascend" in refused(b"5=3=", offsets=[0, 3, 2])
        assert "not at 0" in refused(b"5=3=", offsets=[1, 2, 4])
        assert _same(sc, seq, [(0, 5)], [1], [b"5="])[0] == [(0, 0, 0, 0, 0, 5, 0, 5)]      # and the handle works on


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        bed = sc.refine_bed("chr")
        iv = ribbit_amd.bed_intervals(bed)
        motifs, motif_off = ribbit_amd.bed_motifs(bed)
        pool, off = ribbit_amd.bed_cigars(bed)
        ks = np.diff(motif_off)
        assert len(iv) > 50_000 and len(off) == len(iv) + 1
        rows, sites, observed, obs_off = sc.record_interruptions(iv, ks, pool, off)
        host = ribbit_amd.host_record_interruptions(seq, iv, ks, pool, off)
    assert np.array_equal(rows, host[0]) and np.array_equal(sites, host[1]) and observed == host[2] and np.array_equal(obs_off, host[3])
    assert int(rows["count"].sum()) == len(sites) and np.array_equal(rows["first"], np.concatenate([[0], np.cumsum(rows["count"])[:-1]]))
    # every 499th row's CIGAR, put together again from its slices
    for i in range(0, len(iv), 499):
        mine = [tuple(int(k[f]) for f in ic.SITE_FIELDS) for k in sites[rows["first"][i]:rows["first"][i] + rows["count"][i]]]
        assert ic.rebuilt_cigar(pool, int(off[i]), int(off[i + 1]), mine) == pool[off[i]:off[i + 1]]
    consistent = iv[:, 0].astype(np.int64) + rows["query"] == iv[:, 1]
    print("rows:", len(iv), "interruptions:", len(sites), "rows whose CIGAR does not span them:", int((~consistent).sum()))
    assert int((~consistent).sum()) * 1000 <= len(iv)
    # from the bases alone: inside every match stretch longer than the motif the bases repeat with the motif's period.  The
    # stretches are what the interruptions leave of [s, s + query), row by row
    upper = np.frombuffer(seq.upper(), np.uint8)
    site_ok = consistent[sites["row"]]
    order = np.concatenate([np.flatnonzero(consistent), sites["row"][site_ok]])
    from_ = np.concatenate([iv[consistent, 0], sites["end"][site_ok]])
    to = np.concatenate([iv[consistent, 1], sites["start"][site_ok]])
    by_row_from, by_row_to = np.lexsort((from_, order)), np.lexsort((to, order))
    a, b, k = from_[by_row_from], to[by_row_to], ks[order[by_row_from]]
    assert np.array_equal(order[by_row_from], order[by_row_to]) and (a <= b).all()
    long_ones = np.flatnonzero(b - a > k)
    assert len(long_ones) > 10_000
    for j in long_ones.tolist():
        assert np.array_equal(upper[a[j]:b[j] - k[j]], upper[a[j] + k[j]:b[j]]), (int(a[j]), int(b[j]), int(k[j]))
    # and every site's observed text is the record's bases there
    width = np.diff(obs_off)
    first = np.clip(sites["start"].astype(np.int64), 0, len(seq))
    assert np.array_equal(width, np.clip(np.maximum(sites["end"], first), None, len(seq)) - first)
    assert np.array_equal(width[site_ok], (sites["end"] - sites["start"])[site_ok])      # (a consistent row lies inside the record)
    index = np.repeat(first - obs_off[:-1], width) + np.arange(len(observed))
    assert np.array_equal(np.frombuffer(seq, np.uint8)[index], np.frombuffer(observed, np.uint8))


# ---- end to end
def _other_bed(fa, path):
    path.write_text("".join(f"{name}\t{k * 997}\t{k * 997 + 400}\n" for name, bases in records(fa) if name for k in range(len(bases) // 2000)))


def _expected(fa, bed):
    """the two files: per record, in input order, what the two text functions make of the host twin's decode of the record's BED rows"""
    by_name = rows_by_record(bed)
    site_bed, purity_bed, left_out = b"", b"", 0
    for name, bases in records(fa):
        text = by_name.get(name, "")
        iv = ribbit_amd.bed_intervals(text)
        ks = np.diff(ribbit_amd.bed_motifs(text)[1])
        pool, off = ribbit_amd.bed_cigars(text)
        rows, sites, observed, obs_off = ribbit_amd.host_record_interruptions(bases, iv, ks, pool, off)
        lines, left = ribbit_amd.interruption_text(name, text, iv, rows, sites, pool, observed, obs_off)
        site_bed += lines
        left_out += left
        purity_bed += ribbit_amd.bed_purity_text(text, iv, ks, rows)
    return site_bed.decode(), purity_bed.decode(), left_out


def test_cli_interruption_bed_and_purity_bed(tmp_path):
    fa, other = tmp_path / "in.fa", tmp_path / "other.bed"
    write_nine_records(fa, 300, 77)
    _other_bed(fa, other)
    common = ["-i", fa, "-m", 2, "-M", 30]
    bed0 = tmp_path / "plain.bed"
    _run(common + ["-o", bed0, "--timing", tmp_path / "t0.json"])
    want_bed = bed0.read_text()
    assert "interruptions" not in _stages(tmp_path / "t0.json")
    want_sites, want_purity, left_out = _expected(fa, want_bed)
    assert len(want_purity.splitlines()) == len(want_bed.splitlines()) and len(want_sites.splitlines()) > 100
    assert all(line.startswith(row + "\t") and line.count("\t") == row.count("\t") + 7 for line, row in zip(want_purity.splitlines(), want_bed.splitlines()))
    assert all(line.count("\t") == 8 for line in want_sites.splitlines())
    note = f"ribbit-hip: --interruption-bed: {left_out} rows whose CIGAR does not span the row were left out\n"
    earlier = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
               "--motif-summary", "--compound-bed"]
    runs = [[], ["--jobs", "3"], ["--devices", "0,0", "--jobs", "2"],
            ["--overlap-with", other] + [x for k, option in enumerate(earlier) for x in (option, tmp_path / f"other{k}")]]
    for k, extra in enumerate(runs):
        bed, site, purity, timing = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.sites.bed", tmp_path / f"r{k}.purity.bed", tmp_path / f"t{k + 1}.json"
        r = _run(common + ["-o", bed, "--interruption-bed", site, "--purity-bed", purity, "--timing", timing] + extra)
        assert bed.read_text() == want_bed
        assert site.read_text() == want_sites, extra
        assert purity.read_text() == want_purity, extra
        assert (note in r.stderr) == (left_out > 0) and r.stderr.count("were left out") == (left_out > 0)
        names = list(_stages(timing))
        assert names[-1] == "interruptions" and names.count("interruptions") == 1
    assert list(_stages(tmp_path / "t4.json"))[6:] == ["mask", "repeats", "loci", "density", "overlap", "best", "classes", "compound", "interruptions"]
    # either option alone makes the same file
    _run(common + ["-o", tmp_path / "a.bed", "--purity-bed", tmp_path / "a.purity.bed", "--timing", tmp_path / "ta.json"])
    assert (tmp_path / "a.purity.bed").read_text() == want_purity and list(_stages(tmp_path / "ta.json"))[-1] == "interruptions"
    _run(common + ["-o", tmp_path / "b.bed", "--interruption-bed", tmp_path / "b.sites.bed"])
    assert (tmp_path / "b.sites.bed").read_text() == want_sites
