"""In-silico PCR on the GPU (primer_products.hip through ribbit_hip_record_oligo_sites and ribbit_hip_record_primer_products):
Scanner.record_oligo_sites and Scanner.record_primer_products against the host twins, exactly and field by field, the smaller
cases against the plain statement of the contract (tests/primer_products_contract.py) too, and ribbit-hip --primer-product-bed
end to end."""
import numpy as np
import pytest

import primer_pairs_contract as pp
import primer_products_contract as pq
import primers_contract as pc
import ribbit_amd
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from ribbit_amd.simulate import simulate_sequence, with_random_background

pytestmark = pytest.mark.gpu
TILE = 16384      # bases of one wavefront's tile (device_planes.h); a lane owns 256 of them, a word holds 32
# a launch of the products' kernel has at most 1024 workgroups of 256 lanes, one lane per pair: beyond that the kernel strides
STRIDE_PAIRS = 1024 * 256


def _sites(sc, seq, oligos, fields=None, contract=True, what=None):
    """the device equals the twin, counts, offsets and positions, and, where asked, the contract"""
    prm = ribbit_amd.product_params(**(fields or {}))
    sites, positions = sc.record_oligo_sites(oligos, prm)
    assert sites.dtype == ribbit_amd.OLIGO_SITES_DT and sites.shape == (len(oligos),) and positions.dtype == np.int32
    twin_sites, twin_positions = ribbit_amd.host_record_oligo_sites(seq, oligos, prm)
    for name in sites.dtype.names:
        assert np.array_equal(sites[name], twin_sites[name]), (name, len(seq), what, fields, np.flatnonzero(sites[name] != twin_sites[name])[:5])
    assert np.array_equal(positions, twin_positions), (len(seq), what, fields)
    got = pq.sites_as_lists(sites, positions)
    if contract:
        assert got == pq.contract_sites(seq, oligos, pq.params(**(fields or {}))), (len(seq), what, fields)
    return got


def _rows(tuples):
    return np.array(tuples, dtype=ribbit_amd.PRIMER_PAIRS_DT).reshape(-1)


def _products(sc, seq, pairs, fields=None, contract=True, what=None):
    prm = ribbit_amd.product_params(**(fields or {}))
    got = sc.record_primer_products(pairs, prm)
    assert got.dtype == ribbit_amd.PRIMER_PRODUCTS_DT and got.shape == (len(pairs),)
    twin = ribbit_amd.host_record_primer_products(seq, pairs, prm)
    for name in got.dtype.names:
        assert np.array_equal(got[name], twin[name]), (name, len(seq), what, fields, np.flatnonzero(got[name] != twin[name])[:5])
    got = pq.as_tuples(got)
    if contract:
        assert got == pq.record_primer_products(seq, pp.as_tuples(pairs), pq.params(**(fields or {}))), (len(seq), what, fields)
    return got


def _with(seq: bytes, at: int, letters: bytes) -> bytes:
    return seq[:at] + letters + seq[at + len(letters):]


def _both_strands(oligos):
    return [o for letters in oligos for o in (letters, pp.reverse_complement(letters))]


def _cut(seq: bytes, at: int, k: int) -> str:
    return seq[at:at + k].decode().upper()


@pytest.mark.parametrize("length", (0, 1, 14, 15, 31, 32, 33, 64, 65, 255, 256, 257, TILE - 40, TILE, TILE + 40))
def test_record_lengths_and_windows_at_the_ends(length):
    """oligos of exactly `seed`, 18, 25 and 32 bases whose window starts at 0 and whose window ends at L, on both strands"""
    seq = pc.clean_record(length, length)
    oligos = [_cut(seq, at, k) for k in (15, 18, 25, 32) if k <= length for at in (0, length - k)] or ["ACGTTGCATGCCATGAC"]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _sites(sc, seq, _both_strands(oligos), what="ends")
        if length >= 15:
            assert got[0][2][0] == 0 and got[1][3][0] == 0 and got[2][2][-1] == length - 15 and got[3][3][-1] == length - 15
        else:
            assert got == [(0, 0, [], [])] * 2
        _sites(sc, seq, _both_strands(oligos)[:4], dict(seed=6, max_mismatches=32, max_sites=1024), what="loose")


def test_windows_across_word_lane_and_tile_edges_at_every_offset():
    """every window of 15, 18, 25 and 32 bases that holds positions 31 | 32, 255 | 256 or 16383 | 16384, on both strands"""
    seq = pc.clean_record(TILE + 300, 77)
    oligos, starts = [], []
    for edge in (32, 256, TILE):
        for k in (15, 18, 25, 32):
            for at in range(edge - k + 1, edge):
                oligos.append(_cut(seq, at, k))
                starts.append(at)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _sites(sc, seq, _both_strands(oligos))
    for j, at in enumerate(starts):
        assert at in got[2 * j][2] and at in got[2 * j + 1][3]


@pytest.mark.parametrize("k, start", ((25, 20), (32, 250), (18, TILE - 9), (16, 30)))
def test_each_rule_at_a_word_edge(k, start):
    """a mismatch at the first and at the last base of the seed, exactly d and d + 1 mismatches outside it, an N and a lower-case
    base in the window, max_mismatches 0 and 32, seed 6 and 16: all on a window that crosses a word edge, on both strands"""
    seq = pc.clean_record(TILE + 100, 5).upper()
    o = _cut(seq, start, k)

    def changed(letters, places):
        out = list(letters)
        for j in places:
            out[j] = "ACGT"[("ACGT".index(out[j]) + 1) % 4]
        return "".join(out)

    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        for seed in (6, 15, 16):
            # forward: the window is the oligo, its seed the last `seed` bases; reverse: the window is the oligo's reverse complement q,
            # its seed q's first `seed` bases
            n = min(4, k - seed + 1)
            forward = [o, changed(o, [k - seed]), changed(o, [k - 1])] + [changed(o, range(m)) for m in range(n)]
            reverse = [o, changed(o, [0]), changed(o, [seed - 1])] + [changed(o, range(seed, seed + m)) for m in range(n)]
            oligos = forward + [pp.reverse_complement(q) for q in reverse]
            for d in (0, 2, 32):
                got = _sites(sc, seq, oligos, dict(seed=seed, max_mismatches=d), what=(seed, d))
                for strand, part in ((2, got[:len(forward)]), (3, got[len(forward):])):
                    assert start in part[0][strand] and start not in part[1][strand] and start not in part[2][strand]
                    for m in range(n):
                        assert (start in part[3 + m][strand]) == (m <= d), (seed, d, strand, m)
        # an N loses the site wherever it lies in the window; a lower-case base does not
        for at in (start, start + k // 2, start + k - 1):
            for letter, stays in ((b"N", False), (bytes([seq[at]]).lower(), True)):
                other = _with(seq, at, letter)
                sc.load_record(other)
                got = _sites(sc, other, _both_strands([o]), what=(at, letter))
                assert (start in got[0][2]) == stays == (start in got[1][3])


def test_equal_oligos_shared_seeds_and_a_palindrome():
    seq = pc.clean_record(3000, 11).upper()
    o = _cut(seq, 500, 24)
    sibling = "TGCATGCA"[:6] + o[6:]      # the same seed and most of the rest, another 5' end: six mismatches
    seq = _with(_with(seq, 1200, sibling.encode()), 2000, pq.PALINDROME.encode())
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _sites(sc, seq, [o, sibling, o, pq.PALINDROME, o.lower(), pp.reverse_complement(o)])
        assert got[0] == got[2] == got[4] == (1, 0, [500], []) and got[1] == (1, 0, [1200], []) and got[3] == (1, 1, [2000], [2000]) and got[5] == (0, 1, [], [500])
        loose = _sites(sc, seq, [o, sibling, o], dict(max_mismatches=6))
        assert loose[0] == loose[1] == loose[2] == (2, 0, [500, 1200], [])


@pytest.mark.parametrize("max_sites", (1, 5, 64, 1024))
def test_exactly_max_sites_copies_and_one_more(max_sites):
    """an oligo planted max_sites times has its list, planted once more it has only its count, and so have the products"""
    rs = np.random.RandomState(max_sites)
    o, b = "GATTACAGATTACAGGCT", pp.reverse_complement("CCTGAAGTCTCGGATCAA")
    unit = o.encode() + pc.clean_record(int(rs.randint(3, 30)), 1).upper()
    for copies in (max_sites, max_sites + 1):
        seq = pc.clean_record(40, 2) + unit * copies + b"CCTGAAGTCTCGGATCAA" + pc.clean_record(50, 3)
        last = 40 + len(unit) * (copies - 1)
        with ribbit_amd.Scanner(2, 30) as sc:
            sc.load_record(seq)
            ((f, v, forward, reverse), _) = _sites(sc, seq, [o, b], dict(max_sites=max_sites))
            assert (f, v, reverse) == (copies, 0, []) and (forward == list(range(40, last + 1, len(unit))) if copies == max_sites else forward is None)
            (r,) = _products(sc, seq, _rows([pq.pair_tuple(o, b, last, 40 + len(unit) * copies)]), dict(max_sites=max_sites, max_product=2**31 - 1))
            assert r[:4] == (copies, 0, 0, 1) and (r[4:7] == (copies, 1, 2 * len(unit) + 18 if copies > 1 else 0) if copies == max_sites else r[4:7] == (-1, 0, 0))


def test_a_homopolymer_has_a_site_at_every_position():
    seq = b"A" * 5000
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        got = _sites(sc, seq, ["A" * 18, "T" * 18, "A" * 32], contract=False)
        assert got == [(4983, 0, None, []), (0, 4983, [], None), (4969, 0, None, [])]
        sc.load_record(seq[:1041])
        assert _sites(sc, seq[:1041], ["A" * 18], dict(max_sites=1024), contract=False) == [(1024, 0, list(range(1024)), [])]


def test_the_pinned_values_and_the_product_rules():
    with ribbit_amd.Scanner(2, 30) as sc:
        for (record, a, b, left_start, right_start, fields), want in pq.PINNED.items():
            sc.load_record(record.encode())
            assert _products(sc, record.encode(), _rows([pq.pair_tuple(a, b, left_start, right_start)]), dict(fields)) == [want]
        L, R, RB = pq._L, pq._R, pq._RB
        gap = pc.clean_record(400, 9).upper().decode()
        # a second right site, so that an other product's size == max_product and max_product + 1; then the same for the own
        # product: longer than max_product it is no product, own == 0
        record = (gap[:40] + L + gap[40:100] + R + gap[100:130] + R + gap[130:180]).encode()
        first, second = 40 + 18 + 60, 40 + 18 + 60 + 18 + 30
        own_size, reach = first + 18 - 40, second + 18 - 40
        sc.load_record(record)
        pair = _rows([pq.pair_tuple(L, RB, 40, first)])
        for max_product, want in ((reach, (2, 1, reach)), (reach - 1, (1, 1, 0)), (own_size, (1, 1, 0)), (own_size - 1, (0, 0, 0)), (1, (0, 0, 0)), (2**31 - 1, (2, 1, reach))):
            (r,) = _products(sc, record, pair, dict(max_product=max_product), what=max_product)
            assert r == (1, 0, 0, 2) + want + (0,)
        # a left - left and a right - right product beside the own one, and a pair with a == b
        record = (gap[:40] + L + gap[40:70] + pp.reverse_complement(L) + gap[70:100] + RB + gap[100:130] + R + gap[130:150]).encode()
        sc.load_record(record)
        got = _products(sc, record, _rows([pq.pair_tuple(L, RB, 40, 184), pq.pair_tuple(L, L, 40, 88), pq.pair_tuple(L, RB, 41, 184)]))
        assert got == [(1, 1, 1, 1, 3, 1, 66, 0), (1, 1, 1, 1, 4, 1, 66, 0), (1, 1, 1, 1, 3, 0, 66, 0)]


@pytest.fixture(scope="module")
def backgrounds():
    """(record, rows, targets, the pairs of the first 300 targets) on a random and on a tiled background"""
    out = {}
    tiled, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    for name, seq in (("random", pc.clean_record(60000, 5)), ("tiled", tiled)):
        rs = np.random.RandomState(17)
        rows, targets = pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 2200, longest=60)
        out[name] = (seq, rows, targets, ribbit_amd.host_record_primer_pairs(seq, rows, targets[:300]))
    return out


def test_a_random_background(backgrounds):
    """at the defaults every pair is specific; with a short seed and any number of mismatches other products appear.  The contract's
    own numbers are asserted first: a kernel that finds nothing cannot pass by agreeing with a twin that finds nothing"""
    seq, rows, targets, pairs = backgrounds["random"]
    paired = pairs[pairs["left_start"] >= 0]
    assert len(paired) >= 250
    at_defaults = pq.record_primer_products(seq, pp.as_tuples(pairs))
    assert all(r == (1, 0, 0, 1, 1, 1, 0, 0) for r, p in zip(at_defaults, pairs) if p["left_start"] >= 0)
    seed8 = pq.record_primer_products(seq, pp.as_tuples(pairs), pq.params(seed=8, max_mismatches=32))
    assert sum(r[4] - r[5] > 0 for r in seed8) >= 80
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        assert _products(sc, seq, pairs, contract=False) == at_defaults
        assert _products(sc, seq, pairs, dict(seed=8, max_mismatches=32), contract=False) == seed8
        seed6 = _products(sc, seq, pairs, dict(seed=6, max_mismatches=32))
        assert sum(r[4] - r[5] > 0 for r in seed6) == len(paired)
        # all 2,200 targets against the twin
        every = sc.record_primer_pairs(rows, targets)
        got = _products(sc, seq, every, contract=False)
        assert got[:300] == at_defaults
        # more pairs than one launch has lanes for: the kernel strides
        many = np.concatenate([every] * (STRIDE_PAIRS // len(every) + 1) + [every[::-1]])
        assert len(many) > STRIDE_PAIRS
        again = pq.as_tuples(sc.record_primer_products(many))
        assert again[:2200] == got and again[-4400:-2200] == got and again[-2200:] == got[::-1]
        # the oligos themselves, as given: each primer has its own site
        oligos = [o for r in pp.as_tuples(paired[:50]) for o in pq.oligos_of(r)]
        sites = _sites(sc, seq, oligos)
        assert all(s[:2] == ((1, 0) if j % 2 == 0 else (0, 1)) for j, s in enumerate(sites))


def test_a_tiled_background(backgrounds):
    """every flank recurs at every locus and many primers are the same oligo: the de-duplication, long lists, and a max_sites that
    splits the pairs"""
    seq, rows, targets, pairs = backgrounds["tiled"]
    paired = pairs[pairs["left_start"] >= 0]
    assert len(paired) >= 200
    distinct = {o for r in pp.as_tuples(paired) for o in pq.oligos_of(r)}
    assert len(distinct) < len(paired)      # (fewer oligos than pairs: many are shared)
    # by the contract every pair's longest list has 81 .. 100 sites: at the default max_sites of 64 none has its products, at 98 the
    # pairs split, at least a quarter either way
    assert all(r[4] == -1 for r, p in zip(pq.record_primer_products(seq, pp.as_tuples(pairs)), pairs) if p["left_start"] >= 0)
    want = pq.record_primer_products(seq, pp.as_tuples(pairs), pq.params(max_sites=98))
    assert all(r[4] == -1 or r[4] - r[5] > 0 for r, p in zip(want, pairs) if p["left_start"] >= 0)
    over = sum(r[4] == -1 for r in want)
    assert over >= len(paired) // 4 and len(paired) - over >= len(paired) // 4, (over, len(paired))
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        assert _products(sc, seq, pairs, dict(max_sites=98), contract=False) == want
        _products(sc, seq, pairs)
        _products(sc, seq, pairs, dict(max_sites=1024))
        _products(sc, seq, pairs, dict(max_sites=1), contract=False)
        _sites(sc, seq, sorted(distinct)[:40] + sorted(distinct)[:40])
        every = sc.record_primer_pairs(rows, targets)
        _products(sc, seq, every, contract=False)


def test_between_the_other_row_outputs(backgrounds):
    """products between composition, mask, best, primer and primer pair calls on one handle: every answer stays what it was"""
    seq, rows, targets, _ = backgrounds["random"]
    seq, targets = seq[:20000], targets[targets[:, 0] < 19000][:200]
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_primer_products(_rows([pq.pair_tuple(pq._L, pq._RB, 0, 38)]))
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_oligo_sites([pq._L])
        sc.load_record(seq)
        comp = sc.record_composition(rows, 100)
        pairs = sc.record_primer_pairs(rows, targets)
        first = _products(sc, seq, pairs)
        assert sum(r[5] for r in first) > 100
        assert np.array_equal(sc.record_primer_pairs(rows, targets), pairs) and _products(sc, seq, pairs, contract=False) == first
        assert np.array_equal(sc.record_composition(rows, 100), comp)
        assert sc.mask_record(rows[::2]) == ribbit_amd.host_mask_record(seq, rows[::2])
        oligos = [o for r in pp.as_tuples(pairs[pairs["left_start"] >= 0][:20]) for o in pq.oligos_of(r)]
        sites = _sites(sc, seq, oligos)
        assert _products(sc, seq, pairs, contract=False) == first
        best, _ = sc.record_best(rows)
        assert np.array_equal(best, ribbit_amd.host_record_best(len(seq), rows)[0])
        assert np.array_equal(sc.record_primers(rows, targets), ribbit_amd.host_record_primers(seq, rows, targets))
        assert _sites(sc, seq, oligos, contract=False) == sites and _products(sc, seq, pairs, contract=False) == first
        assert np.array_equal(sc.record_composition(rows, 100), comp) and np.array_equal(sc.record_primer_pairs(rows, targets), pairs)
        # the refusals on a loaded handle
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: max_sites 1025 is outside 1 .. 1024"):
            sc.record_primer_products(pairs, ribbit_amd.product_params(max_sites=1025))
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: oligo 1: 14 bases, not seed 15 .. 32"):
            sc.record_oligo_sites([pq._L, pq._L[:14]])
        # a shorter record on the same handle, and an empty one
        sc.load_record(seq[:900])
        short = sc.record_primer_pairs(rows, targets)
        _products(sc, seq[:900], short)
        _products(sc, seq[:900], pairs, contract=False)      # (pairs of the longer record: their sites are what this record has)
        sc.load_record(b"")
        assert _products(sc, b"", pairs[:5]) == [pq.NO_PRODUCTS] * 5 and _sites(sc, b"", [pq._L]) == [(0, 0, [], [])]
        assert len(sc.record_primer_products(pairs[:0])) == 0 and len(sc.record_oligo_sites([])[0]) == 0


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
        pairs = pp.record_primer_pairs_without_loops(bases, rows.tolist(), rows[chosen].tolist(), pc.params(flank=flank))
        out += pq.product_lines(lines, pairs, pq.record_primer_products(bases, pairs))
    return out


def test_cli_nine_records_and_a_random_background(tmp_path):
    fa = tmp_path / "in.fa"
    write_nine_records(fa, 61, 67)
    seq, truth = simulate_sequence(25000, 23, 2, 30, n_block_rate=0.2, lower_rate=0.2)
    with open(fa, "ab") as fh:
        fh.write(b">random_background\n" + with_random_background(seq, truth, 3) + b"\n")
    bed, products, pairs = tmp_path / "out.bed", tmp_path / "products.bed", tmp_path / "pairs.bed"
    _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--primer-product-bed", products, "--primer-pair-bed", pairs, "--timing", tmp_path / "t.json"])
    got = products.read_text()
    assert got == _expected(fa, bed.read_text(), 200)
    lines = got.splitlines()
    assert len(lines) > 30 and all(len(l.split("\t")) == 38 for l in lines)
    assert ["\t".join(l.split("\t")[:32]) for l in lines] == pairs.read_text().splitlines()
    last = [l.split("\t") for l in lines if l.startswith("random_background\t")]
    assert sum(l[36] == "0" for l in last) > len(last) // 2 and any(l.split("\t")[36] not in ("0", ".") for l in lines)
    stages = list(_stages(tmp_path / "t.json"))
    assert stages[-2:] == ["primer_pairs", "primer_products"] and stages.count("primer_products") == 1
    out = {}
    for jobs in (1, 3):
        b, p = tmp_path / f"bed{jobs}", tmp_path / f"products{jobs}"
        _run(["-i", fa, "-o", b, "-m", 2, "-M", 30, "--primer-product-bed", p, "--primer-product-flank", 90, "--jobs", jobs, "--timing", tmp_path / f"t{jobs}.json"])
        out[jobs] = (b.read_text(), p.read_text())
        assert list(_stages(tmp_path / f"t{jobs}.json"))[-1] == "primer_products" and "primer_pairs" not in _stages(tmp_path / f"t{jobs}.json")
    assert out[1] == out[3] and out[1][0] == bed.read_text()
    assert out[1][1] == _expected(fa, bed.read_text(), 90) != got
    # without the option the key is not there (one record is enough to see that)
    small = tmp_path / "small.fa"
    small.write_bytes(b">random_background\n" + with_random_background(seq, truth, 3) + b"\n")
    _run(["-i", small, "-o", tmp_path / "b.bed", "-m", 2, "-M", 30, "--primer-pair-bed", tmp_path / "p", "--timing", tmp_path / "t0.json"])
    assert "primer_products" not in _stages(tmp_path / "t0.json") and list(_stages(tmp_path / "t0.json"))[-1] == "primer_pairs"
