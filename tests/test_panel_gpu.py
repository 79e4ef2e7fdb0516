"""The primer pairs pooled into multiplex panels, on the GPU (panel.hip through ribbit_hip_panel_pools and
ribbit_hip_debug_panel_conflicts): Scanner.panel_pools against its host twin, exactly, field by field; the conflict matrix as the
kernel leaves it against the plain statement of the contract (tests/panel_contract.py) and against the twin's degrees, at every
tile and chunk edge of the kernel; and ribbit-hip --marker-fasta --marker-bed --panel-bed end to end against the contract applied to
the marker file the tool wrote.
The kernel's shapes (kernels.h): a tile is 64 columns, one matrix word; the words are split evenly over
min(words, max(8, ceil(2048 / words))) column chunks, so a chunk holds one word up to 45 words (2880 pairs) and one or two from 46
words on: 2881 pairs are the fewest that meet a chunk of two words, and a last word of one column with it; from 256 words on
(16,321 pairs) there are 8 chunks, of 32 words and more.  The first fit takes the order through LDS 1,024 keys at a time, and a
key is a row that has a pair: 1,025 such rows are the fewest that fill the tile a second time, 2,049 a third time."""
import numpy as np
import pytest

import panel_contract as pc
import primers_contract as prim
import ribbit_amd
from cli_rows import run as _run, stages as _stages
from panel_cases import check_properties, marker_rows, random_oligo, random_panel, second_assembly, sparse_panel, three_records
from ribbit_amd.simulate import write_fasta

pytestmark = pytest.mark.gpu
PAIRS_DT, DT = ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PANEL_DT
TILE, TARGET_BLOCKS, MIN_CHUNKS = 64, 2048, 8


def chunks_of(n):
    words = (n + TILE - 1) // TILE
    return max(1, min(words, max(MIN_CHUNKS, -(-TARGET_BLOCKS // max(words, 1)))))


def test_the_shapes_this_file_is_written_for():
    assert chunks_of(2880) == 45 == (2880 + 63) // 64 and chunks_of(2881) == 45 < 46 and chunks_of(2945) == 44 and chunks_of(65536) == 8


@pytest.fixture(scope="module")
def sc():
    with ribbit_amd.Scanner(2, 6) as scanner:      # (no record is loaded: the panel needs none)
        yield scanner


def bits_of(words, n):
    """the (n, W) uint64 words as an n x 64 W array of 0 and 1"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").reshape(n, -1) if n else np.zeros((0, 0), np.uint8)


def pooled(sc, pairs, extra=None, sample=None, matrix=True, **fields):
    """the device's pools, which equal the twin's field by field, and its matrix, which has the shape the contract gives it, the
    twin's degrees as row sums and, for the rows `sample` (all of them up to 60), the contract's bits -> (rows, pools, matrix)"""
    arr, prm, n = np.array(pairs, dtype=PAIRS_DT), ribbit_amd.panel_params(**fields), len(pairs)
    got, pools = sc.panel_pools(arr, extra, prm)
    want, want_pools = ribbit_amd.host_panel_pools(arr, extra, prm)
    assert got.dtype == DT == want.dtype and got.shape == want.shape == (n,)
    for name in DT.names:
        assert np.array_equal(got[name], want[name]), (n, fields, name, np.argwhere(got[name] != want[name])[:5].tolist())
    assert pools == want_pools
    check_properties(pairs, pc.as_tuples(got), pools, prm.pool_size)
    if not matrix:      # (above the 8,192 pairs of debug_panel_conflicts)
        return got, pools, None
    words = sc.debug_panel_conflicts(arr, extra, prm)
    assert words.dtype == np.uint64 and words.shape == (n, (n + 63) // 64)
    m = bits_of(words, n)
    assert not m[:, n:].any(), "a column at or beyond n"
    m = m[:, :n]
    has = np.array([pc.has_pair(r) for r in pairs], dtype=bool)
    assert np.array_equal(m, m.T) and not m.diagonal().any() and not m[~has].any() and not m[:, ~has].any()
    assert np.array_equal(m.sum(axis=1), want["conflicts"])
    for p in range(pools):      # no two members of a pool are in conflict
        inside = np.flatnonzero(got["pool"] == p)
        assert not m[np.ix_(inside, inside)].any(), p
    if sample is None and n <= 60:
        sample = list(range(n))
    if sample is not None and len(sample):
        assert len(sample) <= 60
        sub = pc.conflict_matrix([pairs[i] for i in sample], None if extra is None else [extra[i] for i in sample], pc.params(**fields))
        assert np.array_equal(m[np.ix_(sample, sample)], np.array(sub, dtype=np.uint8).reshape(len(sample), len(sample))), (n, fields)
    return got, pools, m


@pytest.mark.parametrize("n", [0, 1, 2, 60, 63, 64, 65, 255, 256, 257])
def test_small_panels_at_the_word_edges(sc, n):
    rs = np.random.RandomState(40 + n)
    pairs, extra = random_panel(n, rs)
    edge = [i for i in (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256) if i < n and pc.has_pair(pairs[i])]
    _, pools, m = pooled(sc, pairs, extra, sample=None if n <= 60 else edge + [int(i) for i in rs.choice(n, 12, replace=False) if pc.has_pair(pairs[i]) and i not in edge])
    assert n < 60 or (pools > 1 and m.any())
    pooled(sc, pairs, None, sample=[] if n > 60 else None)


@pytest.mark.parametrize("n", [2880, 2881, 2945])
def test_panels_at_the_chunk_edges(sc, n):
    rs = np.random.RandomState(n)
    words, chunks = (n + 63) // 64, chunks_of(n)
    firsts = sorted({64 * (words * y // chunks) for y in range(chunks)})      # the first column of every chunk
    two_words = [f for f, g in zip(firsts, firsts[1:] + [64 * words]) if g - f == 128]
    assert (n == 2880) == (not two_words)
    around = {c for f in ([0, 64 * (words - 1)] + two_words[:2] + two_words[-1:]) for c in range(f - 2, f + 130) if 0 <= c < n} | set(range(n - 66, n))
    pairs, extra = sparse_panel(n, rs, around)
    edges = sorted({c for f in two_words[:1] + two_words[-1:] for c in (f - 1, f, f + 63, f + 64, f + 127, f + 128) if 0 <= c < n} | {0, 63, 64, n - 65, n - 2, n - 1})
    sample = edges + [int(i) for i in rs.choice(n, 400, replace=False) if pc.has_pair(pairs[i]) and i not in edges][:40 - len(edges)]
    got, pools, m = pooled(sc, pairs, extra, sample=sample)
    assert pools > 8 and m[edges].any() and m[n - 1].any()


FIT_TILE = 1024      # the keys of the order that the first fit holds in LDS at a time (panel.hip)


@pytest.mark.parametrize("n", [FIT_TILE - 1, FIT_TILE, FIT_TILE + 1, 2 * FIT_TILE + 1])
def test_every_row_with_a_pair_at_the_edges_of_the_first_fits_tile(sc, n):
    # a step of the first fit is a row that has a pair: here all n have one, so the tile of keys is filled again at step 1,024 (and
    # 2,048), with a last tile of 1,023, 0, 1 and 1 keys.  Oligos of 15 .. 18 bases keep the twin's n^2 / 2 tests short.
    rs = np.random.RandomState(n)
    pairs, extra = random_panel(n, rs, none_every=1 << 30, lengths=(15, 19))
    assert all(pc.has_pair(p) for p in pairs)
    sample = [i for i in (0, 1, 63, 64, FIT_TILE - 2, FIT_TILE - 1, FIT_TILE, n - 2, n - 1) if i < n] + [int(i) for i in rs.choice(n, 16, replace=False)]
    # many pools: the defaults fill pools of 8 and every rule refuses
    got, pools, m = pooled(sc, pairs, extra, sample=sorted(set(sample)))
    assert pools > n // 8 and len(set(got["conflicts"].tolist())) > 50
    # few pools: the dimer rule alone, pools without a limit, so the late steps look through the same few pools (the largest panel
    # is left to the defaults: its twin takes seconds)
    if n <= FIT_TILE + 1:
        got, few, m = pooled(sc, pairs, extra, sample=[], size_gap=0, max_cross_product=0, pool_size=65536)
        assert 1 < few < 60 and m.any()


@pytest.mark.parametrize("n,one_in", [(4097, 7), (8192, 7), (16321, 16), (16400, 16)])
def test_chunks_of_three_words_and_more(sc, n, one_in):
    # 4,097 pairs are 65 words in 32 chunks, the first with a chunk of three words; 8,192 are the most whose matrix can be read
    # back; from 16,321 on there are 8 chunks (32 words each, and 33 in the last at 16,400)
    words = (n + 63) // 64
    assert max(words * (y + 1) // chunks_of(n) - words * y // chunks_of(n) for y in range(chunks_of(n))) >= 3 and (chunks_of(n) == 8) == (n >= 16321)
    rs = np.random.RandomState(n)
    pairs, extra = sparse_panel(n, rs, dense=list(range(n - 66, n)) + list(range(130)), one_in=one_in, lengths=(15, 19))
    got, pools, m = pooled(sc, pairs, extra, sample=[], matrix=n <= 8192)
    assert pools > 8 and got["conflicts"][n - 1] > 0


def test_oligos_of_every_length(sc):
    rs = np.random.RandomState(5)
    # 32 against 32 has 63 placements; 15 against 32; every length in between
    longest = [pc.pair(random_oligo(rs, 32), random_oligo(rs, 32), 100 * k, 100 * k + 300) for k in range(24)]
    shortest = [pc.pair(random_oligo(rs, 15), random_oligo(rs, 15), 100 * k, 100 * k + 300) for k in range(24)]
    ladder = [pc.pair(random_oligo(rs, 15 + k), random_oligo(rs, 32 - k), 100 * k, 100 * k + 300) for k in range(18)]
    single = [pc.pair("G", "C", 0, 50), pc.pair("GGGGGGG", "CCCCCCC", 0, 90), pc.pair("C" * 32, "G" * 32, 0, 200), pc.pair("ACGT" * 8, "ACGT" * 8, 0, 300)]
    for pairs in (longest, shortest, ladder, longest[:20] + shortest[:20] + ladder, single):
        _, _, m = pooled(sc, pairs, size_gap=0, max_cross_product=0)
        assert m.any()


def test_rows_without_a_pair_at_the_word_edges(sc):
    rs = np.random.RandomState(6)
    pairs, extra = random_panel(130, rs, none_every=1 << 30)
    for i in (0, 63, 64, 127, 128, 129):
        pairs[i] = pc.NO_PAIR
    got, _, _ = pooled(sc, pairs, extra, sample=[1, 2, 62, 65, 66, 126])
    assert (got["pool"][[0, 63, 64, 127, 128, 129]] == -1).all()
    none = [pc.NO_PAIR] * 70
    got, pools, m = pooled(sc, none, sample=[])
    assert pools == 0 and not m.any()


def test_all_in_conflict_none_in_conflict_and_the_pool_sizes(sc):
    rs = np.random.RandomState(7)
    pairs, extra = random_panel(70, rs, none_every=1 << 30)
    same = [(0, 200, 200)] * 70
    got, pools, m = pooled(sc, pairs, same, sample=[])
    assert pools == 70 and m.sum() == 70 * 69 and got["pool"].tolist() == list(range(70))
    off = dict(max_cross_any=32, max_cross_end=32, size_gap=0, max_cross_product=0)
    for pool_size, want in ((8, 9), (1, 70), (65536, 1), (70, 1), (69, 2)):
        got, pools, m = pooled(sc, pairs, extra, sample=[], pool_size=pool_size, **off)
        assert pools == want == -(-70 // pool_size) and not m.any() and got["pool"].tolist() == [i // pool_size for i in range(70)]
    assert pooled(sc, pairs, extra, sample=[], pool_size=1)[1] == 70


def test_each_rule_alone(sc):
    rs = np.random.RandomState(8)
    pairs, extra = random_panel(100, rs)
    sample = [int(i) for i in range(100) if pc.has_pair(pairs[i])][:30]
    no_dimer, no_size, no_near = dict(max_cross_any=32, max_cross_end=32), dict(size_gap=0), dict(max_cross_product=0)
    sums = {}
    for name, fields in (("dimer", dict(no_size, **no_near)), ("size", dict(no_dimer, **no_near)), ("near", dict(no_dimer, **no_size)), ("all", {})):
        got, _, m = pooled(sc, pairs, extra, sample=sample, **fields)
        sums[name] = m
        if name != "all":
            assert m.any() and np.array_equal(got[name], got["conflicts"]) and not any(got[o].any() for o in ("dimer", "size", "near") if o != name)
    assert np.array_equal(sums["all"], sums["dimer"] | sums["size"] | sums["near"])
    for fields in (dict(max_cross_any=4, max_cross_end=3), dict(max_cross_any=0, max_cross_end=0), dict(max_cross_any=32, max_cross_end=0), dict(max_cross_any=7, max_cross_end=32),
                   dict(size_gap=100000), dict(max_cross_product=1 << 30), dict(max_cross_product=1)):
        pooled(sc, pairs, extra, sample=sample, **fields)


def test_the_pinned_values_and_the_refusals(sc):
    for name, case in pc.pinned_cases().items():
        pairs, extra, fields, _, pools, _ = case
        got, got_pools, _ = pooled(sc, pairs, extra, **fields)
        assert (pc.as_tuples(got), got_pools) == (pc.pinned_rows(case), pools), name
    q = np.array([pc.quiet_pair(0, 0, 100), pc.quiet_pair(1, 0, 200)], dtype=PAIRS_DT)
    with pytest.raises(ribbit_amd.RibbitHipError, match="ribbit_hip error -1: pool_size 0 is outside 1 .. 65536"):
        sc.panel_pools(q, None, ribbit_amd.panel_params(pool_size=0))
    with pytest.raises(ribbit_amd.RibbitHipError, match="ribbit_hip error -1: pair 1: group -2 is below -1"):
        sc.debug_panel_conflicts(q, [(0, 1, 1), (-2, 1, 1)])
    many = np.zeros(pc.MAX_DEBUG_PAIRS + 1, dtype=PAIRS_DT)
    many["left_start"] = -1
    with pytest.raises(ribbit_amd.RibbitHipError, match=r"ribbit_hip error -1: 8193 pairs \(at most 8192\)"):
        sc.debug_panel_conflicts(many)
    rows, pools = sc.panel_pools(many)      # (the pools take them)
    assert pools == 0 and (rows["pool"] == -1).all()


# ---- the tool, end to end
def _penalty(row):
    prm = prim.DEFAULTS
    each = [abs(row[2 + 6 * s] - prm["tm_opt"]) + 10 * abs(row[1 + 6 * s] - prm["opt_length"]) for s in (0, 1)]
    return each[0] + each[1] + abs(row[2] - row[8])


def _expected_panel(marker_text, names, pool_size=8, most=16384):
    rows = marker_rows(marker_text, names)
    taken = [(i, abs(size - row[14])) for i, (row, _, products, size, _) in enumerate(rows) if row is not None and products == "1" and size != row[14]]
    if len(taken) > most:
        taken = sorted(sorted(taken, key=lambda t: (-t[1], _penalty(rows[t[0]][0]), t[0]))[:most])
    pairs = [rows[i][0] for i, _ in taken]
    extra = [(rows[i][1], min(rows[i][0][14], rows[i][3]), max(rows[i][0][14], rows[i][3])) for i, _ in taken]
    panel, pools = pc.panel_pools(pairs, extra, pc.params(pool_size=pool_size))
    return pc.panel_lines("".join(rows[i][4] + "\n" for i, _ in taken), panel, [p[14] for p in pairs]), len(taken), pools


def test_cli_markers_pooled_end_to_end(tmp_path):
    home = three_records()
    names = [name for name, _ in home]
    fa, other_fa = tmp_path / "home.fa", tmp_path / "other.fa"
    write_fasta(str(fa), home, width=70)
    g = tmp_path / "genome0"
    _run(["-i", fa, "-o", tmp_path / "bed0", "-m", 2, "-M", 8, "--primer-genome-bed", g, "--jobs", 1])
    write_fasta(str(other_fa), second_assembly(home, g.read_text()), width=60)
    m1, p1 = tmp_path / "markers1", tmp_path / "panel1"
    _run(["-i", fa, "-o", tmp_path / "bed1", "-m", 2, "-M", 8, "--marker-fasta", other_fa, "--marker-bed", m1, "--panel-bed", p1, "--jobs", 1,
          "--timing", tmp_path / "t1.json"])
    assert list(_stages(tmp_path / "t1.json"))[-3:] == ["primer_genome", "markers", "panel"]
    want, members, pools = _expected_panel(m1.read_text(), names)
    assert p1.read_text() == want and members >= 20 and pools > 1
    got = [l.split("\t") for l in want.splitlines()]
    assert all(len(c) == 36 for c in got) and [int(c[31]) for c in got] == sorted(int(c[31]) for c in got) and max(int(c[31]) for c in got) == pools - 1
    # other pools, fewer markers, the records side by side: the answer does not depend on --jobs
    m2, p2 = tmp_path / "markers2", tmp_path / "panel2"
    _run(["-i", fa, "-o", tmp_path / "bed2", "-m", 2, "-M", 8, "--marker-fasta", other_fa, "--marker-bed", m2, "--panel-bed", p2, "--panel-pool-size", 3, "--panel-max", 15,
          "--jobs", 4, "--devices", "0"])
    assert m2.read_text() == m1.read_text()
    want2, members2, _ = _expected_panel(m1.read_text(), names, 3, 15)
    assert p2.read_text() == want2 and members2 == 15 and want2 != want
