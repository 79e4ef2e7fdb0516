"""The specific primer pairs of a genome on the GPU (primer_specific.hip through ribbit_hip_record_primer_shortlists and
ribbit_hip_record_shortlist_verdicts): Scanner.record_primer_shortlists and Scanner.record_shortlist_verdicts against their host
twins, exactly; lists -> verdicts -> choose against Scanner.record_specific_primer_pairs on one handle; the three pinned genomes
through two loads on one Scanner; and ribbit-hip --primer-genome-bed end to end against the plain statement of the contract
(tests/primer_genome_contract.py)."""
import numpy as np
import pytest

import primer_genome_contract as pg
import primer_specific_contract as ps
import primers_contract as pc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages
from ribbit_amd.simulate import simulate_sequence, with_random_background, write_fasta

pytestmark = pytest.mark.gpu


def _params(prm=None, pair=None, product=None):
    return ribbit_amd.primer_params(**(prm or {})), ribbit_amd.primer_pair_params(**(pair or {})), ribbit_amd.product_params(**(product or {}))


def _same(got, want, dt, what):
    assert got.dtype == dt == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        for name in dt.names:
            assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def _lists(sc, seq, rows, targets, prm=None, pair=None, what=None):
    """the device's shortlists, which equal the twin's"""
    p, q, _ = _params(prm, pair)
    got = sc.record_primer_shortlists(rows, targets, p, q)
    _same(got, ribbit_amd.host_record_primer_shortlists(seq, rows, targets, p, q), ribbit_amd.PRIMER_SHORTLISTS_DT, (what, prm, pair))
    return got


def _verdicts(sc, seq, lists, home, pair=None, product=None, what=None):
    """the device's verdicts on the loaded record `seq`, which equal the twin's"""
    _, q, r = _params(None, pair, product)
    got = sc.record_shortlist_verdicts(lists, home, q, r)
    _same(got, ribbit_amd.host_record_shortlist_verdicts(seq, lists, home, q, r), ribbit_amd.PRIMER_VERDICTS_DT, (what, home, pair, product))
    return got


def _held(lists, side):
    return (lists[side]["start"] >= 0).sum(axis=1)


def _home_record():
    """40,000 bases with a random background, N blocks and lower-case loci, and its loci's neighbourhoods as rows and targets"""
    seq, truth = simulate_sequence(40000, 31, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    seq = with_random_background(seq, truth, 5)
    rs = np.random.RandomState(11)
    rows = [(s, e) for s, e, _, _ in truth]
    targets = rows[:60] + pc.edge_targets(len(seq)) + pc.random_targets(len(seq), rs, 40, longest=60).tolist()
    return seq, rows, targets


def test_the_shortlists_equal_the_twin():
    seq, rows, targets = _home_record()
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        plain = _lists(sc, seq, rows, targets)
        three = _lists(sc, seq, rows, targets, pair=dict(shortlist=3))
        none = _lists(sc, seq, rows, targets, prm=dict(flank=0))
        wide = _lists(sc, seq, rows, targets, prm=dict(flank=1000))
        sc.debug_set_specific_batch(7)
        _same(_lists(sc, seq, rows, targets), plain, ribbit_amd.PRIMER_SHORTLISTS_DT, "batches of 7")
        sc.debug_set_specific_batch(0)
        assert len(_lists(sc, seq, rows, [])) == 0
        sc.load_record(b"")
        empty = _lists(sc, b"", [], [(0, 5), (-3, 2)])
    left, right = _held(plain, "left"), _held(plain, "right")
    assert ((left == 0) != (right == 0)).any() and ((left > 0) & (left < 8)).any() and (left == 8).sum() > 20      # an empty side, fewer than 8, full lists
    assert _held(three, "left").max() == 3 == _held(three, "right").max() and (three["left_passed"] > 3).any()
    assert _held(none, "left").max() == 0 and (none["left_candidates"] == 0).all()
    # flanks of 1,000 bases clipped at both ends of the record: fewer candidates than further inside
    assert wide["left_candidates"][60] < wide["left_candidates"].max() and (wide["left_candidates"] >= plain["left_candidates"]).all()
    assert _held(empty, "left").max() == 0 and empty["left"]["start"].min() == -1


def test_the_verdicts_equal_the_twin_at_home_and_abroad():
    seq, rows, targets = _home_record()
    foreign = pc.clean_record(30000, 5).upper()
    foreign = foreign[:9000] + seq[10000:16000].upper() + foreign[15000:]      # 6,000 bases of the home record: pairs there have products abroad
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        lists = _lists(sc, seq, rows, targets)
        short = _lists(sc, seq, rows, targets, pair=dict(shortlist=3))
        home = _verdicts(sc, seq, lists, 1, what="home")
        as_foreign = _verdicts(sc, seq, lists, 0, what="home as foreign")
        _verdicts(sc, seq, short, 1, pair=dict(shortlist=3), product=dict(seed=12, max_mismatches=0, max_product=300), what="home, other parameters")
        assert len(_verdicts(sc, seq, lists[:0], 1)) == 0
        for batch in (1, 100, 0):
            sc.debug_set_specific_batch(batch)
            _same(sc.record_shortlist_verdicts(lists, 1), home, ribbit_amd.PRIMER_VERDICTS_DT, ("batch", batch))
        sc.load_record(foreign)
        abroad = _verdicts(sc, foreign, lists, 0, what="foreign")
        for nothing in (b"", b"ACGTACGTAC", b"N" * 700):
            sc.load_record(nothing)
            v = _verdicts(sc, nothing, lists, 0, what=nothing[:10])
            assert np.array_equal(v["admissible"], home["admissible"]) and not (v["over"] | v["other"] | v["own"]).any() and not v["forward"].any()
    assert (home["own"] != 0).sum() > 30 and (home["admissible"] != 0).sum() > 30 and not as_foreign["own"].any()
    assert np.array_equal(as_foreign["other"], home["other"] | home["own"])
    assert (abroad["other"] != 0).sum() >= 3 and not abroad["own"].any() and (abroad["other"] == 0).sum() > 30


def test_a_tiled_foreign_record_and_oligos_that_many_targets_share():
    """lists made on a tiled record, where every flank recurs at every locus, so many targets hold the same oligos; judged on another
    record of the same bases: at max_sites 64 lists are too long, at 98 the outcomes split"""
    seq, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    rs = np.random.RandomState(17)
    rows, targets = pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 120, longest=60).tolist()
    targets += targets[:40]      # ... and whole targets a second time
    foreign = b"N" * 100 + seq      # (the same bases as another record, 100 positions further on)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        lists = _lists(sc, seq, rows, targets)
        sc.load_record(foreign)
        at_64 = _verdicts(sc, foreign, lists, 0, what="tiled, 64")
        at_98 = _verdicts(sc, foreign, lists, 0, product=dict(max_sites=98), what="tiled, 98")
        sc.debug_set_specific_batch(50)
        _same(sc.record_shortlist_verdicts(lists, 0, None, ribbit_amd.product_params(max_sites=98)), at_98, ribbit_amd.PRIMER_VERDICTS_DT, "batches of 50")
    oligos = lists["left"][["length", "bases_lo", "bases_hi"]][lists["left"]["start"] >= 0]
    assert len(np.unique(oligos)) < len(oligos) // 4
    assert (at_64["over"] != 0).sum() > 30 and (at_64["forward"].max(axis=1) > 64).sum() > 30
    assert (at_98["over"] != 0).sum() > 10 and (at_98["other"] != 0).sum() > 10
    assert np.array_equal(at_64["forward"], at_98["forward"]) and np.array_equal(at_64["admissible"], at_98["admissible"])


def test_lists_verdicts_and_choice_are_the_specific_call():
    seq = pc.clean_record(30000, 9)
    seq = seq[:12000] + seq[2000:6000] + seq[16000:]      # 4,000 bases a second time: the pairs there have other products
    rs = np.random.RandomState(5)
    rows, targets = pc.random_targets(len(seq), rs, 150, longest=60), pc.random_targets(len(seq), rs, 400, longest=60)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        want = sc.record_specific_primer_pairs(rows, targets)
        lists = sc.record_primer_shortlists(rows, targets)
        got = ribbit_amd.primer_shortlists_choose(lists, sc.record_shortlist_verdicts(lists, 1))
    for g, w, dt in zip(got, want, (ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PRIMER_PRODUCTS_DT, ribbit_amd.PRIMER_SPECIFIC_DT)):
        _same(g, w, dt, dt.names[0])
    place = want[2]["place"]
    assert (place == 0).sum() > 100 and (place > 0).sum() > 5 and (place < 0).sum() > 5


def test_the_three_pinned_genomes_through_two_loads():
    with ribbit_amd.Scanner(2, 30) as sc:
        for name, (home, other) in pg.pinned_genomes().items():
            sc.load_record(home)
            lists = _lists(sc, home, [], [pg.TARGET])
            total = _verdicts(sc, home, lists, 1, what=name)
            sc.load_record(other)
            total = ribbit_amd.primer_verdicts_merge(total, _verdicts(sc, other, lists, 0, what=name))
            pairs, products, specific = (ps.as_tuples(a) for a in ribbit_amd.primer_shortlists_choose(lists, total))
            (p,), (s,) = pairs, specific
            assert (s[:6], (p[0], p[1], p[6], p[7])) == pg.PINNED[name], name
            assert (pairs, products, specific) == pg.genome_specific_primer_pairs([home, other], 0, [], [pg.TARGET], loops=False), name


# ---- end to end
def _ten_records(fa):
    """ten records of 6,000 .. 15,000 bases with random backgrounds, so that a flank is unique unless it is put somewhere else: of the
    loci of record k that lie clear of its ends and of N, the first goes into record k + 1 whole, with both flanks of 200 bases (its
    pairs all have a product there); of the next six the nearest 90, 105 .. 165 bases of either flank go there without the locus
    between them (only the pairs that lie that near have one)"""
    made = []
    for k in range(10):
        seq, truth = simulate_sequence(6000 + 1000 * k, 300 + k, 2, 30, n_block_rate=0.2, lower_rate=0.2)
        made.append((bytearray(with_random_background(seq, truth, 40 + k)), truth))
    for k in range(9):
        seq, truth = made[k]
        clear = [(s, e) for s, e, _, _ in truth if s > 400 and e + 400 < len(seq) and b"N" not in seq[s - 200:e + 200].upper()]
        into = made[k + 1][0]
        s, e = clear[0]
        whole = seq[s - 200:e + 200]
        into[300:300 + len(whole)] = whole
        for j, (s2, e2) in enumerate(clear[1:7]):
            near = 90 + 15 * j
            part = seq[s2 - near:s2] + seq[e2:e2 + near]
            at = len(into) - 500 - 300 * j
            into[at:at + len(part)] = part
    write_fasta(str(fa), [(f"rec{k} description dropped", bytes(seq)) for k, (seq, _) in enumerate(made)], width=70)


def _expected(fa, bed, flank):
    """the file: the contract and the plain formatter applied to the tool's own BED and its best selection per record, in input order"""
    by_name = rows_by_record(bed)
    genome = records(fa)
    out = ""
    for home, (name, bases) in enumerate(genome):
        text = by_name.get(name, "")
        rows = ribbit_amd.bed_intervals(text)
        chosen, _ = ribbit_amd.host_record_best(len(bases), rows)
        lines = ribbit_amd.bed_rows_text(text, chosen).decode()
        out += ps.specific_lines(lines, *pg.genome_specific_primer_pairs([b for _, b in genome], home, rows.tolist(), rows[chosen].tolist(), pc.params(flank=flank), loops=False))
    return out


def _rows_without_a_site_elsewhere(fa, bed):
    """per selected row, in the file's order: none of the 16 oligos of its shortlists has a site in another record (by the twins)"""
    by_name, genome, out = rows_by_record(bed), records(fa), []
    for home, (name, bases) in enumerate(genome):
        rows = ribbit_amd.bed_intervals(by_name.get(name, ""))
        chosen, _ = ribbit_amd.host_record_best(len(bases), rows)
        lists = ribbit_amd.host_record_primer_shortlists(bases, rows, rows[chosen])
        sites = np.zeros(len(lists), np.int64)
        for k, (_, other) in enumerate(genome):
            if k != home:
                v = ribbit_amd.host_record_shortlist_verdicts(other, lists, 0)
                sites += v["forward"].sum(axis=1) + v["reverse"].sum(axis=1)
        out += (sites == 0).tolist()
    return out


def test_cli_ten_records_of_which_some_flanks_recur(tmp_path):
    fa = tmp_path / "in.fa"
    _ten_records(fa)
    b, g, p = tmp_path / "bed1", tmp_path / "genome1", tmp_path / "specific1"
    _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-genome-bed", g, "--primer-specific-bed", p, "--jobs", 1, "--timing", tmp_path / "t1.json"])
    bed, got, specific = b.read_text(), g.read_text(), p.read_text()
    stages = list(_stages(tmp_path / "t1.json"))
    assert stages[-2:] == ["primer_specific", "primer_genome"] and stages.count("primer_genome") == 1
    assert got == _expected(fa, bed, 200)
    lines, alone = [l.split("\t") for l in got.splitlines()], [l.split("\t") for l in specific.splitlines()]
    assert len(lines) == len(alone) > 30 and all(len(l) == 42 for l in lines) and [l[:11] for l in lines] == [l[:11] for l in alone]
    # where no other record holds a site of the row's oligos -- the chosen pair's counts and every verdict are the record's own -- the
    # 42 columns are --primer-specific-bed's; a row never has an earlier place, some have a later one, some lose their pair
    untouched = _rows_without_a_site_elsewhere(fa, bed)
    assert len(untouched) == len(lines) and sum(untouched) > 5 and all(l == a for l, a, u in zip(lines, alone, untouched) if u)
    place = lambda l: 64 if l[38] == "." else int(l[38])
    assert all(place(l) >= place(a) for l, a in zip(lines, alone))
    assert any(place(a) < place(l) < 64 for l, a in zip(lines, alone)) and any(place(a) < 64 == place(l) for l, a in zip(lines, alone))
    assert all(l[29:32] == a[29:32] for l, a in zip(lines, alone))      # (passing candidates and admissible pairs are the record's)
    # four records side by side, the output alone, the devices option: the same files, its stage the last one
    b, g = tmp_path / "bed4", tmp_path / "genome4"
    _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-genome-bed", g, "--jobs", 4, "--devices", "0", "--timing", tmp_path / "t4.json"])
    assert b.read_text() == bed and g.read_text() == got
    stages = list(_stages(tmp_path / "t4.json"))
    assert stages[-1] == "primer_genome" and "primer_specific" not in stages
    # without the option the key is not there (one record is enough to see that)
    small = tmp_path / "small.fa"
    small.write_bytes(b">one\n" + records(fa)[0][1] + b"\n")
    _run(["-i", small, "-o", tmp_path / "b0", "-m", 2, "-M", 30, "--primer-specific-bed", tmp_path / "p0", "--timing", tmp_path / "t0.json"])
    assert "primer_genome" not in _stages(tmp_path / "t0.json") and list(_stages(tmp_path / "t0.json"))[-1] == "primer_specific"
