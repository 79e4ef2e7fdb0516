"""The base composition of rows, flanks and windows on the GPU (composition.hip through ribbit_hip_record_composition and
ribbit_hip_record_base_windows): Scanner.record_composition and Scanner.record_base_windows against the host twins and the plain
statement of the contract (tests/composition_contract.py), exactly, and ribbit-hip --composition-bed / --composition-track end to
end."""
import numpy as np
import pytest

import composition_contract as cc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages
from ribbit_amd.simulate import simulate_sequence, write_fasta

pytestmark = pytest.mark.gpu
# a lane of the block-count kernel takes the B bases of the 8 words a lane of the scan tile owns (composition.hip: COMP_BLOCK)
B = 256
assert B == cc.B
# word, block and tile edges (a tile is 16384 bases, device_planes.h)
LENGTHS = (0, 1, 31, 32, 33, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, 16383, 16384, 16385, 40000)
FLANKS = (0, 1, 31, 32, B - 1, B, 1000, 2**31 - 1)
# a launch has at most 1024 blocks of 256 lanes (composition.hip): beyond that the row kernel and the window kernel stride
STRIDE_LANES = 1024 * 256


def _builds():
    return int(ribbit_amd.load_library().ribbit_debug_composition_prefix_builds())


def _same_rows(sc, seq, rows, flank, what=None, loops=True):
    """the device equals the twin and the contract"""
    got = sc.record_composition(rows, flank)
    assert got.dtype == ribbit_amd.COMPOSITION_DT and got.shape == (len(rows),)
    assert np.array_equal(got, ribbit_amd.host_record_composition(seq, rows, flank)), (len(seq), flank, what)
    if loops:
        assert cc.as_tuples(got) == cc.record_composition(seq, rows, flank), (len(seq), flank, what)
    else:
        assert np.array_equal(cc.as_array(got), cc.record_composition_without_loops(seq, rows, flank)), (len(seq), flank, what)
    return got


def _same_windows(sc, seq, window, loops=True):
    got = sc.record_base_windows(window)
    assert got.dtype == ribbit_amd.BASE_COUNTS_DT and got.shape == (-(-len(seq) // window),)
    assert np.array_equal(got, ribbit_amd.host_record_base_windows(seq, window)), (len(seq), window)
    if loops:
        assert cc.as_tuples(got) == cc.record_base_windows(seq, window), (len(seq), window)
    else:
        assert np.array_equal(cc.as_array(got), cc.record_base_windows_without_loops(seq, window)), (len(seq), window)
    return got


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_sequences_rows_and_flanks(length):
    """every length with every kind of sequence, every edge set and every flank: the tail behind L never leaks into `other`, and
    case is folded"""
    with ribbit_amd.Scanner(2, 30) as sc:
        for name, seq in cc.sequences(length, length):
            before = _builds()
            sc.load_record(seq)
            for what, rows in cc.edge_case_sets(length):
                for flank in FLANKS:
                    # the large sets and lengths by cumulative sums, everything else by the loops
                    _same_rows(sc, seq, rows, flank, (name, what), loops=length <= 2 * B + 1 or len(rows) < 10)
            assert _builds() - before == (1 if length else 0), name


@pytest.mark.parametrize("length", LENGTHS)
def test_lengths_sequences_and_windows(length):
    with ribbit_amd.Scanner(2, 30) as sc:
        for name, seq in cc.sequences(length, length):
            sc.load_record(seq)
            whole = cc.counts(seq, 0, length)
            for window in sorted({w for w in (1, 31, 32, 33, B - 1, B, B + 1, length - 1, length, length + 1, 2**31 - 1) if w >= 1}):
                got = _same_windows(sc, seq, window, loops=length <= 2 * B + 1 or window >= 31)
                assert [int(got[f].sum()) for f in got.dtype.names] == whole, (name, window)


def test_rows_beyond_one_stride():
    """more rows than one launch has lanes: the row kernel strides"""
    rs = np.random.RandomState(44)
    length, many = 1_000_000, 300_000
    assert many > STRIDE_LANES
    seq = next(cc.sequences(length, 5))[1]
    rows = cc.random_rows(length, rs, many, longest=3)      # (short, and half of them empty: they cover a quarter of the record)
    rows[::50_000, 1] += 20_000
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        _same_rows(sc, seq, rows, 1000, loops=False)
        got = _same_rows(sc, seq, rows, 3, loops=False)
    assert (got["left_covered"] > 0).sum() > 1000 and (got["left_covered"] == 0).sum() > 1000 and (got["other"] > 0).sum() > 1000


def test_windows_beyond_one_stride():
    """W = 1 on 300,000 bases: more windows than one launch has lanes, and every window's counts name its one base"""
    length = 300_000
    assert length > STRIDE_LANES
    seq = next(cc.sequences(length, 6))[1]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _same_windows(sc, seq, 1, loops=False)
    kinds = cc.as_array(got)
    assert (kinds.sum(1) == 1).all()
    assert np.array_equal(kinds.argmax(1), cc.kinds_of(seq))


def test_second_call_and_new_record():
    """the same arguments again, other rows, a shorter record, an empty one and the first again: the record's prefix is built on the
    first call after a load and only then"""
    rs = np.random.RandomState(8)
    first_seq, short_seq = next(cc.sequences(20_000, 1))[1], next(cc.sequences(9_000, 2))[1]
    rows = cc.random_rows(20_000, rs, 300, longest=700, reach=50)
    with ribbit_amd.Scanner(2, 30) as sc:
        start = _builds()
        sc.load_record(first_seq)
        assert _builds() == start                                    # (a load alone builds nothing)
        first = _same_rows(sc, first_seq, rows, 100)
        assert _builds() == start + 1
        assert _same_rows(sc, first_seq, rows, 100).tolist() == first.tolist()
        _same_rows(sc, first_seq, rows[:90], 100)
        _same_rows(sc, first_seq, rows, 7)
        windows = _same_windows(sc, first_seq, 1000)
        assert _same_windows(sc, first_seq, 1000).tolist() == windows.tolist()
        _same_windows(sc, first_seq, 999)
        assert _builds() == start + 1                                # other rows, flanks and windows: the same prefix
        sc.load_record(short_seq)
        _same_windows(sc, short_seq, 1000)                           # (the windows first this time)
        shorter = _same_rows(sc, short_seq, rows, 100)
        assert shorter.tolist() != first.tolist()
        assert _builds() == start + 2
        sc.load_record(b"")
        assert _same_rows(sc, b"", rows, 100).tolist() == [(0,) * 13] * len(rows)
        assert len(_same_windows(sc, b"", 1000)) == 0
        assert len(sc.record_composition([], 100)) == 0
        assert _builds() == start + 2                                # (an empty record has no prefix)
        sc.load_record(first_seq)
        assert _same_rows(sc, first_seq, rows, 100).tolist() == first.tolist()
        assert _same_windows(sc, first_seq, 1000).tolist() == windows.tolist()
        assert len(sc.record_composition([], 100)) == 0
        assert _builds() == start + 3


def test_between_the_other_row_outputs():
    """the mask and the overlap of other rows in between, on one handle: the coverage bitmap is theirs then, and is rebuilt"""
    rs = np.random.RandomState(9)
    length = 30_000
    seq = next(cc.sequences(length, 3))[1]
    rows_a, rows_b = cc.random_rows(length, rs, 400, longest=500), cc.random_rows(length, rs, 300, longest=900)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        first = _same_rows(sc, seq, rows_a, 200)
        assert sc.mask_record(rows_b) == ribbit_amd.host_mask_record(seq, rows_b)
        overlap = sc.record_overlap(rows_b, rows_a)
        assert _same_rows(sc, seq, rows_a, 200).tolist() == first.tolist()
        assert sc.mask_record(rows_a) == ribbit_amd.host_mask_record(seq, rows_a)      # (the bitmap is rows_a's now: shared)
        assert sc.record_overlap(rows_b, rows_a)[0].tolist() == overlap[0].tolist()
        assert _same_rows(sc, seq, rows_b, 200).tolist() != first.tolist()
        # the density's covered bases and the flanks' are the same coverage
        density = sc.record_density(rows_a, 1000)
        assert _same_rows(sc, seq, rows_a, 200).tolist() == first.tolist()
        whole = sc.record_composition(np.concatenate([rows_a, [[0, 0], [length, length]]]), length)
        assert int(whole["right_covered"][-2]) == int(density.sum()) == int(whole["left_covered"][-1])


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_composition([(0, 1)], 5)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_base_windows(10)
        sc.load_record(b"ACGT")
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: flank -1 is negative"):
            sc.record_composition([(0, 1)], -1)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: window 0 is below 1"):
            sc.record_base_windows(0)


# ---- end to end
def _expected(fa, bed, flank, window):
    """the two files: the contract and the plain formatters applied to the BED per record, in input order"""
    by_name = rows_by_record(bed)
    comp, track = "", ""
    for name, bases in records(fa):
        text = by_name.get(name, "")
        rows = ribbit_amd.bed_intervals(text).tolist()
        comp += cc.composition_lines(text, cc.record_composition_without_loops(bases, rows, flank).tolist())
        track += cc.window_lines(name, len(bases), window, cc.record_base_windows_without_loops(bases, window).tolist())
    return comp, track


def test_cli_simulated_record(tmp_path):
    seq, _ = simulate_sequence(200_000, 27, 2, 30, lower_rate=0.2)
    seq = bytearray(seq)
    for at, n in ((0, 3), (5_000, 40), (77_777, 1_000), (150_000, 7), (199_990, 10)):      # a few N runs, at both ends too
        seq[at:at + n] = b"N" * n
    seq = bytes(seq)
    fa, bed, comp, track, rep, den = (tmp_path / n for n in ("in.fa", "out.bed", "comp.bed", "comp.track", "rep.fa", "den.bedgraph"))
    write_fasta(str(fa), [("sim description dropped", seq)])
    _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--composition-bed", comp, "--composition-flank", 150, "--composition-track", track, "--repeat-fasta", rep,
          "--flank", 150, "--density-bedgraph", den, "--timing", tmp_path / "t.json"])
    rows = bed.read_text()
    assert len(rows.splitlines()) > 30
    got = comp.read_text()
    want_comp, want_track = _expected(fa, rows, 150, 10000)
    assert got == want_comp
    assert track.read_text() == want_track
    # the first 11 columns are the BED byte for byte
    assert "".join(l.rsplit("\t", 13)[0] + "\n" for l in got.splitlines()) == rows
    assert all(len(l.split("\t")) == 24 for l in got.splitlines())
    # an independent cross-check: the same rows' entries of --repeat-fasta, letters counted in their bodies
    entries = rep.read_text().splitlines()
    assert len(entries) == 2 * len(got.splitlines())
    some_flank_n = some_lower = 0          # (a row itself holds no N: every scan's runs end at one)
    for line, header, body in zip(got.splitlines(), entries[0::2], entries[1::2]):
        a, c, g, t, other, left, left_gc, left_other, _, right, right_gc, right_other, _ = (int(v) for v in line.split("\t")[11:])
        assert header.endswith(f" flank={left},{right}")
        assert len(body) == left + a + c + g + t + other + right
        count = lambda s, letters: sum(s.upper().count(ch) for ch in letters)
        row, lf, rf = body[left:len(body) - right], body[:left], body[len(body) - right:]
        assert (a, c, g, t) == tuple(count(row, ch) for ch in "ACGT") and other == len(row) - count(row, "ACGT")
        assert (left_gc, left_other) == (count(lf, "CG"), len(lf) - count(lf, "ACGT"))
        assert (right_gc, right_other) == (count(rf, "CG"), len(rf) - count(rf, "ACGT"))
        some_flank_n += left_other + right_other > 0
        some_lower += body != body.upper()
    assert some_flank_n and some_lower
    # the track's lines pair with the density file's, and its columns add up to the record
    track_lines, den_lines = track.read_text().splitlines(), den.read_text().splitlines()
    assert [l.split("\t")[:3] for l in track_lines] == [l.split("\t")[:3] for l in den_lines] and len(track_lines) == 20
    sums = [sum(int(l.split("\t")[k]) for l in track_lines) for k in range(3, 8)]
    assert sums == cc.counts(seq, 0, len(seq)) and sums[4] >= 1060
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "composition" and stages.count("composition") == 1
    # one of the two alone
    _run(["-i", fa, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--composition-track", tmp_path / "t2.track", "--composition-window", 777, "--loci-bed",
          tmp_path / "l.bed", "--timing", tmp_path / "t2.json"])
    assert (tmp_path / "t2.track").read_text() == _expected(fa, rows, 150, 777)[1]
    assert list(_stages(tmp_path / "t2.json"))[-2:] == ["loci", "composition"]


def test_cli_three_records_in_flight(tmp_path):
    recs = [("first", simulate_sequence(30_000, 41, 2, 30, n_block_rate=0.3)[0]), ("tiny", b"acgNT"), ("third", simulate_sequence(20_000, 43, 2, 30, lower_rate=0.3)[0])]
    fa = tmp_path / "in.fa"
    write_fasta(str(fa), recs)
    out = {}
    for jobs in (1, 2):
        bed, comp, track = (tmp_path / f"{n}{jobs}" for n in ("bed", "comp", "track"))
        _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--composition-bed", comp, "--composition-track", track, "--composition-window", 4096, "--jobs", jobs])
        out[jobs] = (bed.read_text(), comp.read_text(), track.read_text())
    assert out[1] == out[2]
    want_comp, want_track = _expected(fa, out[1][0], 100, 4096)
    assert out[1][1:] == (want_comp, want_track)
    assert "tiny\t0\t5\t1\t1\t1\t1\t1\n" in want_track
    assert [l.split("\t")[0] for l in want_track.splitlines()] == ["first"] * 8 + ["tiny"] + ["third"] * 5
