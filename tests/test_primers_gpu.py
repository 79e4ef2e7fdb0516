"""Primers in the flanks of chosen rows on the GPU (primers.hip through ribbit_hip_record_primers): Scanner.record_primers against
the host twin and the plain statement of the contract (tests/primers_contract.py), exactly and field by field, and ribbit-hip
--primer-bed end to end."""
import numpy as np
import pytest

import primers_contract as pc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence

pytestmark = pytest.mark.gpu
# a wavefront scans its window in chunks of 64 positions and stages it in words of 32 (primers.hip)
FLANKS = (0, 17, 18, 63, 64, 65, 128, 200, 1000)
SMALL = dict(min_length=5, max_length=8, opt_length=6, tm_min=0, tm_opt=150, tm_max=400, gc_min_percent=20, gc_max_percent=80)
# a launch has at most 1024 workgroups of 4 wavefronts, one wavefront per target and side: beyond 2048 targets the kernel strides
STRIDE_TARGETS = 1024 * 4 // 2


def _same(sc, seq, rows, targets, what=None, **fields):
    """the device equals the twin and the contract"""
    got = sc.record_primers(rows, targets, ribbit_amd.primer_params(**fields))
    assert got.dtype == ribbit_amd.PRIMERS_DT and got.shape == (len(targets),)
    twin = ribbit_amd.host_record_primers(seq, rows, targets, ribbit_amd.primer_params(**fields))
    for name in got.dtype.names:
        assert np.array_equal(got[name], twin[name]), (name, len(seq), what, fields)
    want = pc.record_primers_without_loops(seq, rows, targets, pc.params(**fields))
    assert pc.as_tuples(got) == want, (len(seq), what, fields)
    return want


def _with(seq: bytes, at: int, letters: bytes) -> bytes:
    return seq[:at] + letters + seq[at + len(letters):]


@pytest.mark.parametrize("length", (300, 1000, 2049, 5000))
def test_lengths_flanks_and_edge_targets(length):
    """windows that start or end at 0, at L and at the word edges, at every flank, with the defaults and with small oligos"""
    seq = _with(_with(pc.clean_record(length, length), length // 3, b"NNN"), 40, b"n")
    rows = [(5, 9), (length // 2, length // 2 + 30), (length - 20, length + 5)]
    targets = pc.edge_targets(length)
    found = 0
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        for flank in FLANKS:
            want = _same(sc, seq, rows, targets, flank, flank=flank)
            found += sum(r[0] >= 0 for r in want) + sum(r[6] >= 0 for r in want)
            if flank < 18:
                assert all(r[12:] == (0, 0) for r in want)
            _same(sc, seq, rows, targets, flank, flank=flank, **SMALL)
        _same(sc, seq, rows, targets, flank=1000, min_length=2, max_length=32, opt_length=20, tm_min=0, tm_max=2000, gc_clamp=0, max_run=31)
    assert found > 50


def test_a_blocked_base_at_the_edges_of_a_window():
    """an N, and a base that another row covers, at the first, the last and the 64th position of either window"""
    clean = pc.clean_record(700, 21)
    s, e, flank = 300, 320, 128
    # whatever is not blocked is admissible (16 random bases melt above 0 degrees)
    every = dict(min_length=16, max_length=18, opt_length=17, gc_min_percent=0, gc_max_percent=100, gc_clamp=0, max_run=18, tm_min=0, tm_max=2000)
    spots = {"left": (s - flank, s - 1, s - flank + 63), "right": (e, e + flank - 1, e + 63)}
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(clean)
        free = _same(sc, clean, [(s, e)], [(s, e)], flank=flank, **every)[0]
        assert free[12] == free[13] == sum(flank - k + 1 for k in (16, 17, 18))
        for k, (side, at) in enumerate((side, at) for side in spots for at in spots[side]):
            covered = _same(sc, clean, [(s, e), (at, at + 1)], [(s, e)], (side, at), flank=flank, **every)[0]
            assert covered[12 + k // 3] < free[12 + k // 3] and covered[13 - k // 3] == free[13 - k // 3]
        for side in spots:
            for at in spots[side]:
                seq = _with(clean, at, b"N")
                sc.load_record(seq)
                with_n = _same(sc, seq, [(s, e)], [(s, e)], (side, at), flank=flank, **every)[0]
                covered = pc.record_primers_without_loops(clean, [(s, e), (at, at + 1)], [(s, e)], pc.params(flank=flank, **every))[0]
                assert with_n[12:] == covered[12:]      # (either way the base is blocked)


def test_a_homopolymer_across_a_chunk_edge():
    """runs of exactly max_run and of max_run + 1 equal bases over positions 63 | 64 of a window, at every offset"""
    base = (b"ACGTCAGTGCATGACTCGAT" * 40)[:700]      # (no two equal neighbours)
    s, e, flank = 300, 310, 200
    # nothing but the run rule turns a candidate down (16 bases of this record melt above 0 degrees)
    every = dict(flank=flank, min_length=16, max_length=18, opt_length=17, gc_min_percent=0, gc_max_percent=100, gc_clamp=0, tm_min=0, tm_max=2000)
    full = sum(flank - k + 1 for k in (16, 17, 18))
    with ribbit_amd.Scanner(2, 30) as sc:
        for max_run in (1, 4):
            for side, from_ in (("left", s - flank), ("right", e)):
                for first in range(from_ + 64 - max_run - 1, from_ + 65):
                    counts = []
                    for run in (max_run, max_run + 1):
                        letter = next(ch for ch in b"ACGT" if ch not in (base[first - 1], base[first + run]))      # (the run is no longer than written)
                        seq = _with(base, first, bytes([letter]) * run)
                        sc.load_record(seq)
                        r = _same(sc, seq, [(s, e)], [(s, e)], (side, first, run), max_run=max_run, **every)[0]
                        counts.append(r[12] if side == "left" else r[13])
                    assert counts[1] < counts[0] == full, (max_run, side, first)


def test_the_tie_break():
    unit = b"ACGTGCA"
    seq = unit * 6 + b"N" * 10 + unit * 6
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        (row,) = _same(sc, seq, [], [(42, 52)], flank=42, gc_clamp=0, **dict(SMALL, min_length=7, max_length=7, opt_length=7))
        assert row[12] == row[13] == 36
        # equal penalties seven bases apart: the nearest to the target on either side
        assert 42 - (row[0] + 7) < 7 and row[6] - 52 < 7
        # of two lengths with one penalty and one distance the shorter: |k - opt| is 1 for 6 and for 8, and a Tm range of one value
        # leaves the penalty to the lengths alone where both melt alike
        _same(sc, seq, [], [(42, 52)], flank=42, gc_clamp=0, **dict(SMALL, min_length=6, max_length=8, opt_length=7))


@pytest.fixture(scope="module")
def simulated():
    seq, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    rs = np.random.RandomState(17)
    return seq, pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 2200, longest=60)


def test_random_targets_on_a_simulated_record(simulated):
    """2,200 targets are more than one launch has wavefronts for: the kernel strides.  At the defaults most targets have both primers"""
    seq, rows, targets = simulated
    assert len(targets) > STRIDE_TARGETS
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        want = _same(sc, seq, rows, targets)
        both = sum(r[0] >= 0 and r[6] >= 0 for r in want)
        assert both >= len(targets) // 4, both
        assert sum(r[0] < 0 for r in want) > 10 and len({r[1] for r in want}) > 4
        # the loop form of the contract on a few of them
        assert pc.record_primers(seq, rows, targets[:40]) == want[:40]


@pytest.mark.parametrize("fields", (dict(flank=1000), dict(flank=64, gc_clamp=0, max_run=2), dict(flank=100, **SMALL), dict(flank=300, min_length=12, max_length=32, opt_length=22, tm_min=450, tm_max=700),
                                    dict(tm_min=630, tm_opt=630, tm_max=630)), ids=lambda f: "-".join(f"{k}{v}" for k, v in list(f.items())[:2]))
def test_non_default_parameters_on_the_simulated_record(simulated, fields):
    seq, rows, targets = simulated
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        _same(sc, seq, rows, targets[:700], **fields)
        _same(sc, seq, targets, targets[:700], **fields)      # (the targets among the rows, as the command-line tool has them)


def test_between_the_other_row_outputs(simulated):
    """primers between composition, mask and best calls on one handle: every answer stays what it was, the record's base prefix
    is built once, and the coverage bitmap is rebuilt for whoever brings other rows"""
    seq, rows, targets = simulated
    seq, targets = seq[:20000], targets[targets[:, 0] < 19000][:300]
    other = rows[::2]
    builds = lambda: int(ribbit_amd.load_library().ribbit_debug_composition_prefix_builds())
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        start = builds()
        comp = sc.record_composition(rows, 100)
        first = _same(sc, seq, rows, targets)
        assert np.array_equal(sc.record_composition(rows, 100), comp) and builds() == start + 1
        assert sc.mask_record(other) == ribbit_amd.host_mask_record(seq, other)
        assert _same(sc, seq, rows, targets) == first
        assert sc.mask_record(rows) == ribbit_amd.host_mask_record(seq, rows)      # (the bitmap is the rows' again: shared)
        best, bases = sc.record_best(rows)
        assert np.array_equal(best, ribbit_amd.host_record_best(len(seq), rows)[0])
        assert _same(sc, seq, rows, rows[best]) == pc.record_primers_without_loops(seq, rows, rows[best])
        assert _same(sc, seq, other, targets) != first
        assert np.array_equal(sc.record_composition(rows, 100), comp) and builds() == start + 1
        assert _same(sc, seq, rows, targets) == first
        assert np.array_equal(sc.record_best(rows)[0], best)
        # a shorter record on the same handle, and an empty one
        sc.load_record(seq[:900])
        _same(sc, seq[:900], rows, targets)
        sc.load_record(b"")
        assert _same(sc, b"", rows, targets[:5]) == [pc.NO_PRIMER * 2 + (0, 0)] * 5
        assert len(sc.record_primers(rows, [])) == 0


def test_before_load_and_bad_parameters():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_primers([], [(0, 1)])
        sc.load_record(b"ACGT")
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: flank 1001 is outside 0 .. 1000"):
            sc.record_primers([], [(0, 1)], ribbit_amd.primer_params(flank=1001))
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: max_length 33 is above 32"):
            sc.record_primers([], [(0, 1)], ribbit_amd.primer_params(max_length=33))
        assert pc.as_tuples(sc.record_primers([], [(0, 1)])) == [pc.NO_PRIMER * 2 + (0, 0)]


# ---- end to end
def _expected(fa, bed, flank):
    """the file: the contract and the plain formatter applied to the tool's own BED and its best selection per record, in input order"""
    by_name = rows_by_record(bed)
    out, best_lines = "", ""
    for name, bases in records(fa):
        text = by_name.get(name, "")
        rows = ribbit_amd.bed_intervals(text)
        chosen, _ = ribbit_amd.host_record_best(len(bases), rows)
        lines = ribbit_amd.bed_rows_text(text, chosen).decode()
        best_lines += lines
        out += pc.primer_lines(lines, pc.record_primers_without_loops(bases, rows.tolist(), rows[chosen].tolist(), pc.params(flank=flank)))
    return out, best_lines


def test_cli_nine_records(tmp_path):
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 61, 67)
    bed, primers = tmp_path / "out.bed", tmp_path / "primers.bed"
    _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--primer-bed", primers, "--timing", tmp_path / "t.json"])
    got = primers.read_text()
    want, best_lines = _expected(fa, bed.read_text(), 200)
    assert got == want
    lines = got.splitlines()
    assert len(lines) > 30 and all(len(l.split("\t")) == 22 for l in lines)
    assert "".join(l.rsplit("\t", 11)[0] + "\n" for l in lines) == best_lines
    assert sum(l.split("\t")[19] != "." for l in lines) >= len(lines) // 4
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "primers" and stages.count("primers") == 1 and "best" not in stages
    # beside the outputs that share its selection, records in flight, another flank
    out = {}
    for jobs in (1, 3):
        b, p, best, comp = (tmp_path / f"{n}{jobs}" for n in ("bed", "primers", "best", "compound"))
        _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-bed", p, "--primer-flank", 90, "--best-bed", best, "--compound-bed", comp, "--jobs", jobs,
              "--timing", tmp_path / f"t{jobs}.json"])
        out[jobs] = (b.read_text(), p.read_text(), best.read_text(), comp.read_text())
        assert list(_stages(tmp_path / f"t{jobs}.json"))[-3:] == ["best", "compound", "primers"]
    assert out[1] == out[3] and out[1][0] == bed.read_text()
    want, best_lines = _expected(fa, out[1][0], 90)
    assert out[1][1] == want and out[1][2] == best_lines and want != got
    # without the option the key is not there
    _run(["-i", fa, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--best-bed", tmp_path / "best", "--timing", tmp_path / "t0.json"])
    assert "primers" not in _stages(tmp_path / "t0.json") and list(_stages(tmp_path / "t0.json"))[-1] == "best"
