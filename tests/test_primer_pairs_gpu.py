"""Primer pairs chosen together on the GPU (primer_pairs.hip through ribbit_hip_record_primer_pairs): Scanner.record_primer_pairs
against the host twin, exactly and field by field, the smaller cases against the plain statement of the contract
(tests/primer_pairs_contract.py) too, and ribbit-hip --primer-pair-bed end to end."""
import numpy as np
import pytest

import primer_pairs_contract as pp
import primers_contract as pc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence

pytestmark = pytest.mark.gpu
# a wavefront scans its window in chunks of 64 positions, stages it in words of 32 and deals its starts to 64 lanes (primer_pairs.hip)
FLANKS = (0, 17, 200, 1000)
SMALL = dict(min_length=5, max_length=8, opt_length=6, tm_min=0, tm_opt=150, tm_max=400, gc_min_percent=20, gc_max_percent=80)
SMALL_PAIR = dict(max_self_any=3, max_self_end=2, max_hairpin=2, max_pair_any=3, max_pair_end=2, max_tm_difference=60)
# whatever is not blocked is admissible: only the pair's own limits turn a candidate down
EVERY = dict(min_length=16, max_length=18, opt_length=17, gc_min_percent=0, gc_max_percent=100, gc_clamp=0, max_run=18, tm_min=0, tm_max=2000)
NO_PAIR = pc.NO_PRIMER * 2 + (0,) * 13
# a launch has at most 1024 workgroups of 4 wavefronts, one wavefront per target: beyond 4096 targets the kernel strides
STRIDE_TARGETS = 1024 * 4


def _same(sc, seq, rows, targets, what=None, fields=None, pair=None, contract=True):
    """the device equals the twin and, where asked, the contract"""
    prm, prs = ribbit_amd.primer_params(**(fields or {})), ribbit_amd.primer_pair_params(**(pair or {}))
    got = sc.record_primer_pairs(rows, targets, prm, prs)
    assert got.dtype == ribbit_amd.PRIMER_PAIRS_DT and got.shape == (len(targets),)
    twin = ribbit_amd.host_record_primer_pairs(seq, rows, targets, prm, prs)
    for name in got.dtype.names:
        assert np.array_equal(got[name], twin[name]), (name, len(seq), what, fields, pair, np.flatnonzero(got[name] != twin[name])[:5])
    got = pp.as_tuples(got)
    if contract:
        assert got == pp.record_primer_pairs_without_loops(seq, rows, targets, pc.params(**(fields or {})), pp.pair_params(**(pair or {}))), (len(seq), what, fields, pair)
    return got


def _with(seq: bytes, at: int, letters: bytes) -> bytes:
    return seq[:at] + letters + seq[at + len(letters):]


@pytest.mark.parametrize("length", (0, 1, 17, 64, 65, 1000))
def test_lengths_flanks_and_edge_targets(length):
    """windows that start or end at 0, at L and at the word edges, at every flank, with the defaults and with small oligos"""
    seq = pc.clean_record(length, length)
    if length == 1000:
        seq = _with(_with(seq, length // 3, b"NNN"), 40, b"n")
    rows = [(5, 9), (length // 2, length // 2 + 30), (length - 20, length + 5)]
    targets = pc.edge_targets(length)
    found = 0
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        for flank in FLANKS:
            found += sum(r[0] >= 0 for r in _same(sc, seq, rows, targets, flank, dict(flank=flank)))
            found += sum(r[0] >= 0 for r in _same(sc, seq, rows, targets, flank, dict(SMALL, flank=flank), SMALL_PAIR))
    assert found > 0 if length == 1000 else found == 0 if length <= 17 else True


def test_a_blocked_base_at_the_edges_of_a_window():
    """an N, and a base that another row covers, at the first, the last and the 64th position of either window"""
    clean = pc.clean_record(700, 21)
    s, e, flank = 300, 320, 128
    spots = {"left": (s - flank, s - 1, s - flank + 63), "right": (e, e + flank - 1, e + 63)}
    fields = dict(EVERY, flank=flank)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(clean)
        free = _same(sc, clean, [(s, e)], [(s, e)], fields=fields)[0]
        assert free[25] == free[26] == sum(flank - k + 1 for k in (16, 17, 18)) and 0 < free[27] < free[25] and 0 < free[28] < free[26]
        for k, (side, at) in enumerate((side, at) for side in spots for at in spots[side]):
            covered = _same(sc, clean, [(s, e), (at, at + 1)], [(s, e)], (side, at), fields)[0]
            assert covered[25 + k // 3] < free[25 + k // 3] and covered[26 - k // 3] == free[26 - k // 3] and covered[28 - k // 3] == free[28 - k // 3]
        for side in spots:
            for at in spots[side]:
                seq = _with(clean, at, b"N")
                sc.load_record(seq)
                with_n = _same(sc, seq, [(s, e)], [(s, e)], (side, at), fields)[0]
                covered = pp.record_primer_pairs_without_loops(clean, [(s, e), (at, at + 1)], [(s, e)], pc.params(**fields), pp.PAIR_DEFAULTS)[0]
                assert with_n[25:] == covered[25:]      # (either way the base is blocked)


@pytest.mark.parametrize("motif", (b"GGATCC", b"ACGTTGCAACGT", b"AAAAAA"), ids=lambda m: m.decode())
def test_a_palindrome_and_a_homopolymer_across_a_chunk_edge(motif):
    """a stretch that binds to itself (or, the homopolymer, to nothing) over positions 63 | 64 of a window, at every offset: the
    admissible candidates stay what they were, and those that hold a palindrome whole fail max_self_any = its length - 1"""
    base = (b"ACGTCAGTGCATGACTCGAT" * 40)[:700]
    s, e, flank = 300, 310, 200
    fields, pair = dict(EVERY, flank=flank), dict(max_self_any=len(motif) - 1, max_self_end=32, max_hairpin=32)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(base)
        plain = _same(sc, base, [(s, e)], [(s, e)], fields=fields, pair=pair)[0]
        for side, from_ in (("left", s - flank), ("right", e)):
            for first in range(from_ + 64 - len(motif) - 1, from_ + 66):
                seq = _with(base, first, motif)
                sc.load_record(seq)
                r = _same(sc, seq, [(s, e)], [(s, e)], (side, first), fields, pair)[0]
                assert r[25:27] == plain[25:27]
                if motif != b"AAAAAA":      # (a palindrome of 2 h bases binds to itself over all of them: the candidates that hold it whole fail)
                    assert (r[27] < r[25]) if side == "left" else (r[28] < r[26])
                # the defaults on the same record
                _same(sc, seq, [(s, e)], [(s, e)], (side, first), dict(flank=flank))
    assert motif == b"AAAAAA" or ribbit_amd.oligo_duplex(motif, motif)[0] == len(motif)


def test_the_shortlist_and_windows_with_few_candidates():
    """shortlists of 1, 3 and 8; a right window with fewer passing candidates than the shortlist, with one and with none"""
    seq = pc.clean_record(900, 1000)
    s, e = 440, 470
    three = [(300, 320), (s, e), (560, 600)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        ranks = set()
        for shortlist in (1, 3, 8):
            for r in _same(sc, seq, three, three, shortlist, pair=dict(shortlist=shortlist)):
                assert r[29] == min(shortlist, r[27]) * min(shortlist, r[28]) and r[15] < shortlist and r[16] < shortlist
                ranks.add((shortlist, r[15], r[16]))
        assert (8, 0, 6) in ranks and len({k for k in ranks if k[0] == 8}) > 1
        # nothing turns a candidate of 18 bases down but the room: a right window of w bases holds w - 17 of them
        fields, loose = dict(EVERY, min_length=18, opt_length=18, flank=100), dict(pp.LOOSE, shortlist=8)
        for room, passed in ((17, 0), (18, 1), (20, 3), (24, 7), (25, 8), (30, 13)):
            (r,) = _same(sc, seq, [(e + room, e + 150)], [(s, e)], room, fields, loose)
            assert r[28] == r[26] == passed and r[29] == 8 * min(8, passed) and (r[0] >= 0) == (passed > 0)
        (r,) = _same(sc, seq, [(s - 150, s - 17)], [(s, e)], "left", fields, loose)
        assert r[:25] == NO_PAIR and r[25:] == (0, 83, 0, 83, 0, 0, 0)


@pytest.fixture(scope="module")
def simulated():
    seq, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    rs = np.random.RandomState(17)
    rows, targets = pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 2200, longest=60)
    return seq, rows, targets, pp.record_primer_pairs_without_loops(seq, rows, targets[:600])


def test_random_targets_on_a_simulated_record(simulated):
    """2,200 targets against the twin and 600 of them against the contract, by which at least half of them have a pair at the
    defaults: a kernel that finds nothing cannot pass by agreeing with a twin that finds nothing"""
    seq, rows, targets, want = simulated
    paired = sum(r[0] >= 0 for r in want)
    assert paired >= len(want) // 2, paired
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _same(sc, seq, rows, targets, contract=False)
        assert got[:600] == want
        assert sum(r[0] < 0 for r in got) > 10 and len({r[1] for r in got}) > 4 and len({(r[15], r[16]) for r in got}) > 8
        # more targets than one launch has wavefronts for: the kernel strides
        many = np.concatenate([targets, targets[::-1], targets[:100]])
        assert len(many) > STRIDE_TARGETS
        again = pp.as_tuples(sc.record_primer_pairs(rows, many))
        assert again[:2200] == got and again[2200:4400] == got[::-1] and again[4400:] == got[:100]


@pytest.mark.parametrize("fields, pair", ((dict(flank=1000), {}), (dict(flank=64, gc_clamp=0, max_run=2), dict(shortlist=3)), (dict(SMALL, flank=100), SMALL_PAIR),
                                          (dict(flank=300, min_length=12, max_length=32, opt_length=22, tm_min=450, tm_max=700), dict(max_hairpin=5, max_self_any=6)),
                                          ({}, dict(max_self_any=2)), ({}, dict(max_self_any=32)), ({}, dict(max_self_end=1)), ({}, dict(max_self_end=32)),
                                          ({}, dict(max_hairpin=0)), ({}, dict(max_hairpin=32)), ({}, dict(max_pair_any=2)), ({}, dict(max_pair_any=32)),
                                          ({}, dict(max_pair_end=0)), ({}, dict(max_pair_end=32)), ({}, dict(max_tm_difference=0)), ({}, dict(max_tm_difference=2000)),
                                          ({}, pp.LOOSE)), ids=lambda f: "-".join(f"{k}{v}" for k, v in list(f.items())[:2]) or "defaults")
def test_non_default_parameters_on_the_simulated_record(simulated, fields, pair):
    seq, rows, targets, _ = simulated
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _same(sc, seq, rows, targets[:300], fields=fields, pair=pair, contract=False)
        assert got[:60] == pp.record_primer_pairs_without_loops(seq, rows, targets[:60], pc.params(**fields), pp.pair_params(**pair))
        _same(sc, seq, targets, targets[:300], fields=fields, pair=pair, contract=False)      # (the targets among the rows, as the command-line tool has them)
        if pair == pp.LOOSE:
            alone = sc.record_primers(rows, targets[:300])
            for r, a in zip(got, pc.as_tuples(alone)):
                assert pp.primers_of(r) == a if a[0] >= 0 and a[6] >= 0 else r[:25] == NO_PAIR and r[25:27] == a[12:]


def test_between_the_other_row_outputs(simulated):
    """primer pairs between composition, mask, best and record_primers calls on one handle: every answer stays what it was"""
    seq, rows, targets, _ = simulated
    seq, targets = seq[:20000], targets[targets[:, 0] < 19000][:200]
    other = rows[::2]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        comp = sc.record_composition(rows, 100)
        first = _same(sc, seq, rows, targets, contract=False)
        alone = sc.record_primers(rows, targets)
        assert np.array_equal(alone, ribbit_amd.host_record_primers(seq, rows, targets))
        assert _same(sc, seq, rows, targets, contract=False) == first
        assert np.array_equal(sc.record_composition(rows, 100), comp)
        assert sc.mask_record(other) == ribbit_amd.host_mask_record(seq, other)
        assert _same(sc, seq, rows, targets, contract=False) == first
        assert sc.mask_record(rows) == ribbit_amd.host_mask_record(seq, rows)      # (the bitmap is the rows' again: shared)
        best, _ = sc.record_best(rows)
        assert np.array_equal(best, ribbit_amd.host_record_best(len(seq), rows)[0])
        _same(sc, seq, rows, rows[best], contract=False)
        assert _same(sc, seq, other, targets, contract=False) != first
        assert np.array_equal(sc.record_primers(rows, targets), alone) and np.array_equal(sc.record_composition(rows, 100), comp)
        assert _same(sc, seq, rows, targets, contract=False) == first
        assert np.array_equal(sc.record_best(rows)[0], best)
        # a shorter record on the same handle, and an empty one
        sc.load_record(seq[:900])
        _same(sc, seq[:900], rows, targets)
        sc.load_record(b"")
        assert _same(sc, b"", rows, targets[:5]) == [NO_PAIR + (0,) * 7] * 5
        assert len(sc.record_primer_pairs(rows, [])) == 0


def test_before_load_and_bad_parameters():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_primer_pairs([], [(0, 1)])
        sc.load_record(b"ACGT")
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: flank 1001 is outside 0 .. 1000"):
            sc.record_primer_pairs([], [(0, 1)], ribbit_amd.primer_params(flank=1001))
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: shortlist 9 is outside 1 .. 8"):
            sc.record_primer_pairs([], [(0, 1)], None, ribbit_amd.primer_pair_params(shortlist=9))
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: max_pair_end 33 is outside 0 .. 32"):
            sc.record_primer_pairs([], [(0, 1)], None, ribbit_amd.primer_pair_params(max_pair_end=33))
        assert pp.as_tuples(sc.record_primer_pairs([], [(0, 1)])) == [NO_PAIR + (0,) * 7]


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
        out += pp.pair_lines(lines, pp.record_primer_pairs_without_loops(bases, rows.tolist(), rows[chosen].tolist(), pc.params(flank=flank)))
    return out, best_lines


def test_cli_nine_records(tmp_path):
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 61, 67)
    bed, pairs = tmp_path / "out.bed", tmp_path / "pairs.bed"
    _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--primer-pair-bed", pairs, "--timing", tmp_path / "t.json"])
    got = pairs.read_text()
    want, best_lines = _expected(fa, bed.read_text(), 200)
    assert got == want
    lines = got.splitlines()
    assert len(lines) > 30 and all(len(l.split("\t")) == 32 for l in lines)
    assert "".join(l.rsplit("\t", 21)[0] + "\n" for l in lines) == best_lines
    assert any(l.split("\t")[19] != "." for l in lines)
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "primer_pairs" and stages.count("primer_pairs") == 1 and "best" not in stages and "primers" not in stages
    # beside the outputs that share its selection, records in flight, another flank
    out = {}
    for jobs in (1, 3):
        b, p, q, best, comp = (tmp_path / f"{n}{jobs}" for n in ("bed", "pairs", "primers", "best", "compound"))
        _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-pair-bed", p, "--primer-pair-flank", 90, "--primer-bed", q, "--best-bed", best, "--compound-bed", comp,
              "--jobs", jobs, "--timing", tmp_path / f"t{jobs}.json"])
        out[jobs] = (b.read_text(), p.read_text(), q.read_text(), best.read_text(), comp.read_text())
        assert list(_stages(tmp_path / f"t{jobs}.json"))[-4:] == ["best", "compound", "primers", "primer_pairs"]
    assert out[1] == out[3] and out[1][0] == bed.read_text()
    want, best_lines = _expected(fa, out[1][0], 90)
    assert out[1][1] == want and out[1][3] == best_lines and want != got
    # --primer-bed beside it keeps its own flank and its 22 columns
    assert all(len(l.split("\t")) == 22 for l in out[1][2].splitlines()) and len(out[1][2].splitlines()) == len(lines)
    # without the option the key is not there
    _run(["-i", fa, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--primer-bed", tmp_path / "p", "--timing", tmp_path / "t0.json"])
    assert "primer_pairs" not in _stages(tmp_path / "t0.json") and list(_stages(tmp_path / "t0.json"))[-1] == "primers"
