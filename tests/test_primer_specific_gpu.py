"""The specific primer pairs on the GPU (primer_specific.hip through ribbit_hip_record_specific_primer_pairs):
Scanner.record_specific_primer_pairs against the host twin, exactly and field by field in all three records, for every target of
every case; the smaller cases against the plain statement of the contract (tests/primer_specific_contract.py) too; against
Scanner.record_primer_pairs and Scanner.record_primer_products on the same handle; and ribbit-hip --primer-specific-bed end to end."""
import numpy as np
import pytest

import primer_pairs_contract as pp
import primer_products_contract as pq
import primer_specific_contract as ps
import primers_contract as pc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence, with_random_background

pytestmark = pytest.mark.gpu
TILE = 16384      # bases of one wavefront's tile of the site scan (device_planes.h)
# a launch of the walk has at most 1024 workgroups of 4 wavefronts, one wavefront per target: beyond that the kernel strides
STRIDE_TARGETS = 1024 * 4


def _params(prm, pair, product):
    return ribbit_amd.primer_params(**(prm or {})), ribbit_amd.primer_pair_params(**(pair or {})), ribbit_amd.product_params(**(product or {}))


def _check(sc, seq, rows, targets, prm=None, pair=None, product=None, contract=False, what=None):
    """the device equals the twin in all three records for every target and, where asked, the contract -> the three lists of tuples"""
    args = _params(prm, pair, product)
    got = sc.record_specific_primer_pairs(rows, targets, *args)
    twin = ribbit_amd.host_record_specific_primer_pairs(seq, rows, targets, *args)
    for g, t, dt in zip(got, twin, (ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PRIMER_PRODUCTS_DT, ribbit_amd.PRIMER_SPECIFIC_DT)):
        assert g.dtype == dt and g.shape == (len(targets),)
        for name in dt.names:
            assert np.array_equal(g[name], t[name]), (name, len(seq), what, prm, pair, product, np.flatnonzero(g[name] != t[name])[:5])
    out = tuple(ps.as_tuples(a) for a in got)
    if contract:
        want = ps.record_specific_primer_pairs(seq, rows, targets, pc.params(**(prm or {})), pp.pair_params(**(pair or {})), pq.params(**(product or {})), loops=False)
        assert out == want, (len(seq), what, prm, pair, product)
    return out


def test_the_five_constructed_records():
    seen = set()
    with ribbit_amd.Scanner(2, 30) as sc:
        for name, (record, fields) in ps.constructed().items():
            sc.load_record(record)
            pairs, products, summaries = _check(sc, record, [], [ps.TARGET], product=fields, contract=True, what=name)
            (s,), (p,) = summaries, pairs
            assert (s[:6], (p[0], p[1], p[6], p[7])) == ps.PINNED[name], name
            seen |= {"first" if s[0] == 0 else "later" if s[0] > 0 else "none with other" if s[4] > 0 else "none", "over" if s[3] > 0 else ""}
    assert {"first", "later", "none with other", "over"} <= seen      # (or the test would pass without a pair ever being passed over)


def test_record_lengths_with_targets_at_both_ends():
    """flanks clipped to nothing, sides with fewer than 8 passing candidates and sides with none, records shorter than a primer"""
    clipped = few = none_one_side = paired = 0
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in (0, 17, 18, 40, 255, 256, 257, TILE - 40, TILE, TILE + 40):
            seq = pc.clean_record(length, length)
            targets = [(s, e) for s, e in pc.edge_targets(length)]
            sc.load_record(seq)
            pairs, _, summaries = _check(sc, seq, [(5, 9)], targets, contract=length <= 257, what="ends")
            for (s, e), p, m in zip(targets, pairs, summaries):
                clipped += min(max(s, 0), length) == 0 or min(max(e, 0), length) == length
                few += 0 < p[27] < 8 or 0 < p[28] < 8
                none_one_side += (p[27] == 0) != (p[28] == 0)
                paired += m[0] >= 0
                assert length >= 40 or m[:6] == (-1, 0, 0, 0, 0, 0)
    assert clipped > 20 and few > 0 and none_one_side > 0 and paired > 10, (clipped, few, none_one_side, paired)


def test_a_copied_primer_window_across_the_tile_boundary():
    """the best pair's left window a second time across positions TILE - 1 | TILE and its right window 60 bases behind: the site scan
    finds a site that two tiles share, and the pair in place 0 is passed over"""
    seq = pc.clean_record(TILE + 600, 21).upper()
    target = (TILE - 2000, TILE - 1960)
    best = pp.as_tuples(ribbit_amd.host_record_primer_pairs(seq, [], [target]))[0]
    assert best[0] >= 0
    left, right = seq[best[0]:best[0] + best[1]], seq[best[6]:best[6] + best[7]]
    at = TILE - len(left) // 2
    seq = seq[:at] + left + seq[at + len(left):]
    seq = seq[:at + len(left) + 60] + right + seq[at + len(left) + 60 + len(right):]
    assert len(seq) == TILE + 600
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        _, products, summaries = _check(sc, seq, [], [target, (TILE - 30, TILE + 10)], contract=True)
        assert summaries[0][0] > 0 and summaries[0][5] > 0 and summaries[0][4] > 0 and products[0][0] + products[0][3] >= 2


@pytest.mark.parametrize("pair", (dict(shortlist=1), dict(shortlist=3), dict(shortlist=8), pp.LOOSE, dict(pp.LOOSE, shortlist=8),
                                  dict(max_self_any=3, max_self_end=2, max_hairpin=2, max_pair_any=3, max_pair_end=2, max_tm_difference=10)))
def test_shortlists_and_pair_limits(pair):
    record, _ = ps.constructed()["best pair copied"]
    rs = np.random.RandomState(3)
    targets = [ps.TARGET] + pc.random_targets(len(record), rs, 12, longest=60).tolist()
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(record)
        pairs, _, summaries = _check(sc, record, [(100, 140)], targets, pair=pair, contract=True)
    assert all(p[29] <= pair.get("shortlist", 8) ** 2 for p in pairs) and any(s[1] > 0 for s in summaries)
    if pair.get("shortlist") == 1:
        assert summaries[0][:5] == (-1, 1, 0, 0, 1)      # (the only pair is the copied one: there is no other to fall back to)


def test_batches_do_not_change_the_result():
    record, _ = ps.constructed()["best pair copied"]
    targets = [ps.TARGET, (700, 730), (0, 10), (2500, 2560), (3990, 4000)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(record)
        whole = _check(sc, record, [], targets, contract=True)
        for batch in (2, 1, 5, 4):      # 2 + 2 + 1, one by one, exactly one batch, 4 + 1
            sc.debug_set_specific_batch(batch)
            assert _check(sc, record, [], targets) == whole, batch
        sc.debug_set_specific_batch(0)
        assert _check(sc, record, [], targets) == whole
    assert whole[2][0][0] > 0 and sum(s[0] >= 0 for s in whole[2]) >= 3


def test_more_targets_than_one_launch_has_wavefronts():
    record, _ = ps.constructed()["best pair copied"]
    n = STRIDE_TARGETS + 4
    targets = [ps.TARGET, (700, 730)] * (n // 2)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(record)
        first = _check(sc, record, [], targets[:2], contract=True)
        got = sc.record_specific_primer_pairs([], targets)
    assert len(got[0]) == n > STRIDE_TARGETS
    for arr, two in zip(got, first):
        tuples = ps.as_tuples(arr)
        assert tuples[0::2] == [two[0]] * (n // 2) and tuples[1::2] == [two[1]] * (n // 2)


def test_consistent_with_the_pair_and_the_product_calls():
    seq = pc.clean_record(30000, 9)
    seq = seq[:12000] + seq[2000:6000] + seq[16000:]      # 4,000 bases a second time: the pairs there have other products
    rs = np.random.RandomState(5)
    rows, targets = pc.random_targets(len(seq), rs, 150, longest=60), pc.random_targets(len(seq), rs, 400, longest=60)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        pairs, products, specific = sc.record_specific_primer_pairs(rows, targets)
        best = sc.record_primer_pairs(rows, targets)
        best_products = sc.record_primer_products(best)
        again = sc.record_primer_products(pairs)
        _check(sc, seq, rows, targets[:60])
    first = specific["place"] == 0
    assert first.sum() > 100 and (specific["place"] > 0).sum() > 5 and (specific["place"] < 0).sum() > 5
    for name in ribbit_amd.PRIMER_PAIRS_DT.names:
        assert np.array_equal(pairs[name][first], best[name][first]), name
    for name in ribbit_amd.PRIMER_PRODUCTS_DT.names:
        assert np.array_equal(again[name], products[name]), name
    chosen = specific["place"] >= 0
    assert np.array_equal(chosen, pairs["left_start"] >= 0) and np.all((products["products"] - products["own"])[chosen] == 0) and np.all(products["own"][chosen] == 1)
    admissible = best["left_start"] >= 0
    assert np.array_equal(admissible, specific["pairs_admissible"] > 0) and np.array_equal(best["pairs_admissible"], specific["pairs_admissible"])
    want = np.where(best_products["products"] < 0, -1, best_products["products"] - best_products["own"])
    assert np.array_equal(specific["first_products"], np.where(admissible, want, 0))
    assert np.array_equal(specific["pairs_specific"] + specific["pairs_over"] + specific["pairs_other"], specific["pairs_admissible"])


def test_a_tiled_background():
    """every flank recurs at every locus: at the default max_sites the lists are too long, every pair of all but a few targets is
    over and those targets have no pair (by the twin one target of the 250 keeps a pair, in a flank that does not recur); at 98 the
    outcomes split"""
    seq, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    rs = np.random.RandomState(17)
    rows, targets = pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 250, longest=60)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        _, _, summaries = _check(sc, seq, rows, targets)
        all_over = [s for s in summaries if s[1] > 0 and s[3] == s[1]]
        assert len(all_over) > 200 and all(s[0] == -1 and s[5] == -1 for s in all_over) and sum(s[0] >= 0 for s in summaries) < 5
        _, _, split = _check(sc, seq, rows, targets, product=dict(max_sites=98))
        assert sum(s[3] > 0 for s in split) > 30 and sum(s[4] > 0 for s in split) > 30
        sc.debug_set_specific_batch(100)
        assert _check(sc, seq, rows, targets, product=dict(max_sites=98))[2] == split


# ---- end to end
def _expected(fa, bed, flank):
    """the file: the contracts and the plain formatters applied to the tool's own BED and its best selection per record, in input order"""
    by_name = rows_by_record(bed)
    out = ""
    for name, bases in records(fa):
        text = by_name.get(name, "")
        rows = ribbit_amd.bed_intervals(text)
        chosen, _ = ribbit_amd.host_record_best(len(bases), rows)
        lines = ribbit_amd.bed_rows_text(text, chosen).decode()
        out += ps.specific_lines(lines, *ps.record_specific_primer_pairs(bases, rows.tolist(), rows[chosen].tolist(), pc.params(flank=flank), loops=False))
    return out


def test_cli_nine_records_and_a_random_background(tmp_path):
    """the nine records are tiled, so their pairs are over or have other products; the tenth has a random background, where most
    targets keep the pair in place 0"""
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 61, 67)
    seq, truth = simulate_sequence(25000, 23, 2, 30, n_block_rate=0.2, lower_rate=0.2)
    with open(fa, "ab") as fh:
        fh.write(b">random_background\n" + with_random_background(seq, truth, 3) + b"\n")
    out = {}
    for jobs in (1, 4):
        b, p, q = tmp_path / f"bed{jobs}", tmp_path / f"specific{jobs}", tmp_path / f"products{jobs}"
        _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-specific-bed", p, "--primer-product-bed", q, "--jobs", jobs, "--timing", tmp_path / f"t{jobs}.json"])
        out[jobs] = (b.read_text(), p.read_text(), q.read_text())
        stages = list(_stages(tmp_path / f"t{jobs}.json"))
        assert stages[-2:] == ["primer_products", "primer_specific"] and stages.count("primer_specific") == 1
    assert out[1] == out[4]
    bed, got, products = out[1]
    assert got == _expected(fa, bed, 200)
    lines, with_products = [l.split("\t") for l in got.splitlines()], [l.split("\t") for l in products.splitlines()]
    assert len(lines) == len(with_products) > 10 and all(len(l) == 42 for l in lines)
    # where the pair in place 0 is taken the first 38 columns are --primer-product-bed's
    assert all(l[:38] == w for l, w in zip(lines, with_products) if l[38] == "0")
    last = [l for l in lines if l[0] == "random_background"]
    assert sum(l[38] == "0" for l in last) > len(last) // 2 and any(l[38] == "." and l[39:] != ["0", "0", "0"] for l in lines)
    # alone, at another flank: the same BED, another answer, and its stage the last one
    b, p = tmp_path / "bed", tmp_path / "specific"
    _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-specific-bed", p, "--primer-specific-flank", 90, "--timing", tmp_path / "t.json"])
    assert b.read_text() == bed and p.read_text() == _expected(fa, bed, 90) != got
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-1] == "primer_specific" and "primer_products" not in stages
    # without the option the key is not there (one record is enough to see that)
    small = tmp_path / "small.fa"
    small.write_bytes(b">random_background\n" + with_random_background(seq, truth, 3) + b"\n")
    _run(["-i", small, "-o", tmp_path / "b0", "-m", 2, "-M", 30, "--primer-product-bed", tmp_path / "q0", "--timing", tmp_path / "t0.json"])
    assert "primer_specific" not in _stages(tmp_path / "t0.json") and list(_stages(tmp_path / "t0.json"))[-1] == "primer_products"
