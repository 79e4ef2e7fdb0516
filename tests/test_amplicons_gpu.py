"""Every chosen primer pair typed on another record, on the GPU (amplicons.hip through ribbit_hip_record_pair_amplicons):
Scanner.record_pair_amplicons against its host twin, exactly, field by field, at home and abroad, on constructed tracts at the
word and tile edges of the planes, in batches; and ribbit-hip --marker-fasta --marker-bed end to end against the plain statement of
the contract (tests/amplicons_contract.py)."""
import numpy as np
import pytest

import amplicons_contract as ac
import primer_pairs_contract as pp
import primer_products_contract as prc
import primers_contract as pc
import ribbit_amd
from cli_rows import records, run as _run, stages as _stages
from ribbit_amd.simulate import _mutate, _primitive_motif, simulate_sequence, with_random_background, write_fasta

pytestmark = pytest.mark.gpu
DT = ribbit_amd.PAIR_AMPLICONS_DT
PAIR = prc.pair_tuple(ac.A, ac.B, 0, 0)
NO_PAIR = (-1, 0, 0, 0, 0, 0) * 2 + (0,) * 20
TILE_BASES = 16384      # a wavefront's tile of the planes (device_planes.h)


def _same(got, want, dt, what):
    assert got.dtype == dt == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        for name in dt.names:
            assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def _typed(sc, seq, pairs, motifs, label=0, what=None, **fields):
    """the device's amplicons on the loaded record `seq`, which equal the twin's"""
    prm = ribbit_amd.product_params(**fields)
    got = sc.record_pair_amplicons(pairs, motifs, label, prm)
    _same(got, ribbit_amd.host_record_pair_amplicons(seq, pairs, motifs, label, prm), DT, (what, label, fields))
    return got


def _reverse_complement(seq: bytes) -> bytes:
    return seq[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def _home_record():
    """40,000 bases with a random background, N blocks and lower-case loci; its loci as rows; as targets the loci, each with its
    motif, then the record's edges and 60 random stretches with the motif CA"""
    seq, truth = simulate_sequence(40000, 31, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    seq = with_random_background(seq, truth, 5)
    rows = [(s, e) for s, e, _, _ in truth]
    targets = rows + pc.edge_targets(len(seq)) + pc.random_targets(len(seq), np.random.RandomState(11), 60, longest=60).tolist()
    return seq, rows, targets, [motif.upper() for _, _, _, motif in truth] + ["CA"] * (len(targets) - len(rows))


def test_home_abroad_and_the_other_strand_equal_the_twin():
    seq, rows, targets, motifs = _home_record()
    foreign = pc.clean_record(30000, 6).upper()
    foreign = foreign[:9000] + seq[10000:16000].upper() + foreign[15000:]      # 6,000 bases of the home record: pairs there have a product abroad
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        pairs = sc.record_primer_pairs(rows, targets)
        home = _typed(sc, seq, pairs, motifs, 4, "home")
        _typed(sc, seq, pairs, motifs, 0, "home, other parameters", seed=12, max_mismatches=0, max_product=300)
        assert len(_typed(sc, seq, pairs[:0], [], 0, "no pairs")) == 0
        for batch in (1, 7, 0):
            sc.debug_set_specific_batch(batch)
            _same(sc.record_pair_amplicons(pairs, motifs, 4), home, DT, ("batch", batch))
        sc.load_record(foreign)
        abroad = _typed(sc, foreign, pairs, motifs, 1, "foreign")
        other_strand = _reverse_complement(seq)
        sc.load_record(other_strand)
        turned = _typed(sc, other_strand, pairs, motifs, 2, "the reverse complement")
        for nothing in (b"", b"ACGTACGTAC", b"N" * 700):
            sc.load_record(nothing)
            a = _typed(sc, nothing, pairs, motifs, 0, nothing[:10])
            assert not a["products"].any() and (a["record"] == -1).all() and (a["tract_end"] == -1).all()
    has, loci = pairs["left_start"] >= 0, np.arange(len(pairs)) < len(rows)
    assert has.sum() > 40 and (~has).sum() > 3 and (home["record"][~has] == -1).all() and not home["left_forward"][~has].any()
    one = home["products"] == 1
    assert (one == has).all() and (home["record"][one] == 4).all()
    # at home the first product is the designed one; a locus holds a tract of its motif as given, a random stretch a short one of CA or TG or none
    assert np.array_equal(home["start"][one], pairs["left_start"][one]) and np.array_equal(home["end"][one] - home["start"][one], pairs["product"][one])
    assert (home["forward_of"][one] == 0).all() and (home["reverse_of"][one] == 1).all()
    held = one & (home["tract_start"] >= 0)
    assert (held & loci).sum() > 10 and not home["tract_strand"][loci].any() and (home["tract_end"] - home["tract_start"])[held & loci].min() >= 12
    assert (held & ~loci).sum() > 5 and (one & ~held).sum() > 5 and home["tract_strand"][~loci].sum() > 2
    # abroad only the pairs of the copied stretch have a product, 10,000 - 9,000 bases further left
    there = abroad["products"] == 1
    assert 3 <= there.sum() < one.sum() and (abroad["record"][there] == 1).all() and np.array_equal(abroad["start"][there], home["start"][there] - 1000)
    assert np.array_equal(abroad["tract_end"][there] - abroad["tract_start"][there], home["tract_end"][there] - home["tract_start"][there])
    # on the other strand the primers change places and the tract its strand
    assert np.array_equal(turned["products"], home["products"]) and (turned["forward_of"][one] == 1).all() and (turned["reverse_of"][one] == 0).all()
    assert np.array_equal(turned["start"][one], len(seq) - home["end"][one]) and np.array_equal(turned["tract_start"] >= 0, home["tract_start"] >= 0)
    assert np.array_equal(turned["tract_end"][held] - turned["tract_start"][held], home["tract_end"][held] - home["tract_start"][held])
    assert (turned["tract_strand"][held & loci] == 1).sum() > 10


def test_the_pinned_values_on_the_device():
    with ribbit_amd.Scanner(2, 30) as sc:
        for (record, motif), value in ac.PINNED.items():
            sc.load_record(record.encode())
            got = _typed(sc, record.encode(), np.array([PAIR, NO_PAIR], dtype=ribbit_amd.PRIMER_PAIRS_DT), [motif, "ACGT"], 5, (record, motif))
            assert ac.as_tuples(got) == [ac.pinned_fields(value, 5), ac.NO_PAIR], (record, motif)


def _filler(n, rs):
    return "".join(rs.choice(list("ACGT"), n))


@pytest.mark.parametrize("m", [1, 2, 31, 32, 33, 65, 100])
def test_tracts_across_word_and_tile_edges(m):
    """one product whose inner part is longer than 64 words and crosses a tile edge of the planes; tracts of the motif and of its
    reverse complement placed so that they start, end and cross at word and tile edges, the longest of them behind shorter ones"""
    rs = np.random.RandomState(500 + m)
    motif = "".join(rs.choice(list("ACGT"), m)) if m > 2 else ("A" if m == 1 else "CA")
    other = pp.reverse_complement(motif)
    lead = TILE_BASES - 1500      # the product starts 1,500 bases before the tile edge
    units = lambda w, n, k: ((w[k % m:] + w[:k % m]) * (n // m + 2))[:n]
    with ribbit_amd.Scanner(2, 30) as sc:
        for shift in (0, 1, 31):
            body = list(_filler(5000, rs))
            def put(at, text):
                body[at:at + len(text)] = text
            inner0 = lead + len(ac.LP) + shift      # the inner part's first base in the record
            edge = TILE_BASES - inner0              # the tile edge, in the body
            put(0, units(motif, 2 * m + 3, 1))                                    # at the inner part's first base
            put(edge - (edge % 32) - 32 - m, units(other, 3 * m + 40, 2))         # across word edges before the tile edge
            put(edge - m - 7, units(motif, 2 * m + 11, 3))                        # across the tile edge
            put(edge + 2100, units(other, 4 * m + 170, 5))                        # the longest, more than 64 words further on
            put(5000 - 2 * m - 1, units(motif, 2 * m + 1, 0))                     # up to the inner part's last base
            record = ("N" * shift + _filler(lead, rs) + ac.LP + "".join(body) + ac.RP + _filler(300, rs)).encode()
            if shift == 1:
                record = record.lower()
            pair = np.array([PAIR], dtype=ribbit_amd.PRIMER_PAIRS_DT)
            sc.load_record(record)
            a = ac.as_tuples(_typed(sc, record, pair, [motif], 0, (m, shift), max_product=6000))[0]
            assert ac.as_tuples(_typed(sc, record, pair, [motif], 0, (m, shift, "the largest product"), max_product=5036))[0] == a
            assert _typed(sc, record, pair, [motif], 0, (m, shift, "one base short"), max_product=5035)["products"][0] == 0
            assert a[4] == 1 and a[10:12] == (inner0, inner0 + 5000) and a[13] - a[12] >= 4 * m + 170, (m, shift, a)
            assert a[12] >= inner0 + edge + 2000 and (a[14] == 1 or other == motif), (m, shift, a)
            # the same inner part without the longest tract: one of the shorter ones, which lie at the edges
            cut = record[:inner0 + edge + 2000] + record[inner0 + edge + 2100 + 4 * m + 170 + 100:]
            sc.load_record(cut)
            b = ac.as_tuples(_typed(sc, cut, pair, [motif], 0, (m, shift, "without the longest"), max_product=6000))[0]
            assert b[4] == 1 and 2 * m <= b[13] - b[12] < 4 * m + 170, (m, shift, b)


def test_a_tiled_foreign_record_is_over():
    seq, _ = simulate_sequence(60000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    rs = np.random.RandomState(17)
    rows, targets = pc.random_targets(len(seq), rs, 300, longest=60), pc.random_targets(len(seq), rs, 120, longest=60)
    motifs = ["CA"] * len(targets)
    foreign = b"N" * 100 + seq
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(seq)
        pairs = sc.record_primer_pairs(rows, targets)
        sc.load_record(foreign)
        at_64 = _typed(sc, foreign, pairs, motifs, 0, "tiled, 64")
        at_1024 = _typed(sc, foreign, pairs, motifs, 0, "tiled, 1024", max_sites=1024)
        sc.debug_set_specific_batch(50)
        _same(sc.record_pair_amplicons(pairs, motifs, 0, ribbit_amd.product_params(max_sites=1024)), at_1024, DT, "batches of 50")
    has = pairs["left_start"] >= 0
    assert has.sum() > 30 and (at_64["products"][has] == -1).sum() > 30 and (at_64["left_forward"] > 64).sum() > 30
    assert (at_64["record"][at_64["products"] <= 0] == -1).all() and not at_64["products"][~has].any()
    assert (at_1024["products"] > 1).sum() > 30 and np.array_equal(at_64["left_forward"], at_1024["left_forward"])


# ---- end to end
def _three_records():
    """three records of about 20 kb: 30 loci each as the simulator makes them (motifs of 2 .. 8 bases, 85 to 95 % pure, one in five
    in lower case), 450 .. 700 random bases between them and an N block before one in five"""
    made = []
    for k in range(3):
        rs = np.random.RandomState(700 + k)
        parts = []
        for _ in range(30):
            parts.append(bytes(rs.choice(list(b"ACGT"), rs.randint(450, 701)).tolist()))
            if rs.random_sample() < 0.2:
                parts.append(b"N" * rs.randint(1, 201))
            m = int(rs.randint(2, 9))
            units = int(rs.randint(8, 25))
            locus = _mutate(rs, _primitive_motif(rs, m) * units, m, units, 0.85, 0.95)
            parts.append(locus.lower() if rs.random_sample() < 0.2 else locus)
        parts.append(bytes(rs.choice(list(b"ACGT"), 500).tolist()))
        made.append((f"home{k}", b"".join(parts)))
    return made


def _chosen(genome_bed: str):
    """the lines of --primer-genome-bed as (record name, row start, row end, motif, the row of 32 values or None, the first 11 columns)"""
    out = []
    for line in genome_bed.splitlines():
        c = line.split("\t")
        assert len(c) == 42
        row = None
        if c[11] != ".":
            row = ()
            for start, end, letters, tm, right in ((c[11], c[12], c[13], c[14], False), (c[15], c[16], c[17], c[18], True)):
                forward = pp.reverse_complement(letters) if right else letters
                bases = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(forward))
                row += (int(start), int(end) - int(start), int(tm.replace(".", "")), 0, pp._i32(bases & 0xffffffff), pp._i32(bases >> 32))
            row += (0, 0, int(c[19])) + (0,) * 17
        out.append((c[0], int(c[1]), int(c[2]), c[3], row, "\t".join(c[:11])))
    return out


def _second_assembly(home, chosen):
    """the home records as another individual's: of the rows with a pair, record by record, one in four keeps its length, one is
    contracted and two are expanded by whole units in their middle; one locus is deleted with its primers; one left primer loses its
    3' base; one pair's stretch lies a second time behind another record; one left primer lies 70 more times behind a record; the
    second record is reverse-complemented and the records change places -> (the records, {(name, row start): bases added}, per
    record every (position, bases added), per record the stretches that were changed in another way)"""
    rs = np.random.RandomState(3)
    filler = lambda n: bytes(rs.choice(list(b"ACGT"), n).tolist())
    special = {("home0", 2): "deleted", ("home0", 7): "many", ("home1", 6): "twice", ("home2", 5): "three prime"}
    made, added, tails = {}, {}, {name: b"" for name, _ in home}
    edits, spoiled = {name: [] for name, _ in home}, {name: [] for name, _ in home}
    for name, bases in home:
        with_pair = [r for r in chosen if r[0] == name and r[4] is not None]
        assert len(with_pair) > 8
        seq = bytearray(bases)
        for j, (_, s, e, motif, row, _) in reversed(list(enumerate(with_pair))):      # (from the right, so that the positions to the left stay)
            left_start, left_end, right_end = row[0], row[0] + row[1], row[6] + row[7]
            stretch = bytes(bases[left_start:right_end]).upper()
            what = special.get((name, j))
            if what == "deleted":
                del seq[left_start:right_end]
                spoiled[name].append((left_start, right_end))
            elif what == "three prime":
                spoiled[name].append((left_start, left_end))
                seq[left_end - 1:left_end] = b"A" if stretch[row[1] - 1:row[1]] != b"A" else b"C"
            elif what == "twice":
                tails["home2"] += filler(300) + stretch
            elif what == "many":
                tails["home0"] += b"".join(filler(10) + stretch[:row[1]] for _ in range(70))
            k, m, mid = 1 + j % 3, len(motif), (s + e) // 2
            if what or j % 4 == 3:
                continue
            if j % 4 == 2:
                if e - s > k * m + 2 * m:
                    del seq[mid:mid + k * m]
                    added[(name, s)] = -k * m
                    edits[name].append((mid, -k * m))
                continue
            seq[mid:mid] = (motif * k).encode()
            added[(name, s)] = k * m
            edits[name].append((mid, k * m))
        made[name] = bytes(seq)
    made = {name: bases + tails[name] + (filler(200) if tails[name] else b"") for name, bases in made.items()}
    return [("other2", made["home2"]), ("other0", made["home0"]), ("other1", _reverse_complement(made["home1"]))], (added, edits, spoiled)


def _expected_markers(chosen, other):
    """the contract applied to the tool's own selection -> (the file, the amplicons)"""
    pairs = [r[4] if r[4] is not None else NO_PAIR for r in chosen]
    amplicons = ac.genome_amplicons([bases for _, bases in other], pairs, [r[3] for r in chosen])
    return ac.marker_lines("".join(r[5] + "\n" for r in chosen), pairs, amplicons, [name for name, _ in other]), amplicons


def _check_markers(chosen, other, added, text):
    want, amplicons = _expected_markers(chosen, other)
    assert text == want
    # on the contract's side: enough rows with one product of another size, and every other outcome
    moved = sum(1 for r, a in zip(chosen, amplicons) if r[4] is not None and a[4] == 1 and a[7] - a[6] != r[4][14])
    outcomes = {("no pair" if r[4] is None else "over" if a[4] < 0 else min(a[4], 2)) for r, a in zip(chosen, amplicons)}
    assert moved >= 20 and outcomes == {"no pair", "over", 0, 1, 2}, (moved, outcomes)
    # without the contract: a row with k m bases more or fewer in its middle has a product that much longer or shorter, on the strand
    # its record has in the other assembly
    # (a short row nearby may lie inside the same product: all changes between the two primers count; a product that holds a stretch
    # changed in another way is left out)
    added, edits, spoiled = added
    lines = {(c[0], int(c[1])): c for c in (l.split("\t") for l in text.splitlines())}
    seen = 0
    for name, start, _, _, row, _ in chosen:
        c = lines[(name, start)]
        if (name, start) not in added or c[20] != "1":
            continue
        left, right = row[0], row[6] + row[7]
        if any(lo < right and left < hi for lo, hi in spoiled[name]):
            continue
        assert int(c[26]) == sum(bases for at, bases in edits[name] if left <= at < right), c
        assert c[24] == ("-" if name == "home1" else "+") and c[21] == "other" + name[4], c
        seen += 1
    assert seen >= 10 and sum(1 for v in added.values() if v < 0) >= 3
    return moved


def test_cli_three_records_typed_on_a_derived_assembly(tmp_path):
    home = _three_records()
    fa, other_fa = tmp_path / "home.fa", tmp_path / "other.fa"
    write_fasta(str(fa), [(name + " description dropped", bases) for name, bases in home], width=70)
    b, g = tmp_path / "bed0", tmp_path / "genome0"
    _run(["-i", fa, "-o", b, "-m", 2, "-M", 8, "--primer-genome-bed", g, "--jobs", 1])
    chosen = _chosen(g.read_text())
    other, added = _second_assembly(home, chosen)
    write_fasta(str(other_fa), [(name + " of another individual", bases) for name, bases in other], width=60)
    assert [(n, s) for n, s in records(other_fa)] == other
    # both files, one record at a time
    b1, g1, m1 = tmp_path / "bed1", tmp_path / "genome1", tmp_path / "markers1"
    _run(["-i", fa, "-o", b1, "-m", 2, "-M", 8, "--primer-genome-bed", g1, "--marker-fasta", other_fa, "--marker-bed", m1, "--jobs", 1, "--timing", tmp_path / "t1.json"])
    assert b1.read_text() == b.read_text() and g1.read_text() == g.read_text()
    stages = list(_stages(tmp_path / "t1.json"))
    assert stages[-2:] == ["primer_genome", "markers"]
    _check_markers(chosen, other, added, m1.read_text())
    # the markers alone, three records side by side: the selection is made all the same
    b4, m4 = tmp_path / "bed4", tmp_path / "markers4"
    _run(["-i", fa, "-o", b4, "-m", 2, "-M", 8, "--marker-bed", m4, "--marker-fasta", other_fa, "--jobs", 4, "--devices", "0", "--timing", tmp_path / "t4.json"])
    assert b4.read_text() == b.read_text() and m4.read_text() == m1.read_text()
    assert list(_stages(tmp_path / "t4.json"))[-2:] == ["primer_genome", "markers"]
    # without the options the key is not there
    _run(["-i", fa, "-o", tmp_path / "b5", "-m", 2, "-M", 8, "--primer-genome-bed", tmp_path / "g5", "--timing", tmp_path / "t5.json"])
    assert "markers" not in _stages(tmp_path / "t5.json") and (tmp_path / "g5").read_text() == g.read_text()
