"""The specific primer pairs of a genome without a GPU: the three genomes whose values include/ribbit_hip.h pins, through the plain
statement (tests/primer_genome_contract.py) and through host twins -> merge -> choose, field by field; one record against the
specific primer pairs; several records against their concatenation; max_sites per record; the sum's laws; every refusal; and
ribbit-hip's handling of --primer-genome-bed and --primer-genome-flank up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import primer_genome_contract as pg
import primer_pairs_contract as pp
import primer_products_contract as pq
import primer_specific_contract as ps
import primers_contract as pc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed", "--nearest-bed", "--nearest-other-bed", "--composition-bed",
                   "--composition-track", "--primer-bed", "--primer-pair-bed", "--primer-product-bed", "--primer-specific-bed"]
MOSTLY_BASES = b"ACGTacgt" * 40 + b"NnRYx-"


def _params(prm=None, pair=None, product=None):
    return ribbit_amd.primer_params(**(prm or {})), ribbit_amd.primer_pair_params(**(pair or {})), ribbit_amd.product_params(**(product or {}))


def _lists(seq, rows, targets, prm=None, pair=None):
    p, q, _ = _params(prm, pair)
    got = ribbit_amd.host_record_primer_shortlists(seq, rows, targets, p, q)
    assert got.dtype == ribbit_amd.PRIMER_SHORTLISTS_DT and got.shape == (len(targets),)
    return got


def _verdicts(seq, lists, home, pair=None, product=None):
    _, q, r = _params(None, pair, product)
    got = ribbit_amd.host_record_shortlist_verdicts(seq, lists, home, q, r)
    assert got.dtype == ribbit_amd.PRIMER_VERDICTS_DT and got.shape == (len(lists),)
    return got


def _verdict_tuples(v):
    return [tuple(tuple(int(x) for x in f) if isinstance(f, np.ndarray) else int(f) for f in r) for r in v]


def _genome(records, home, rows, targets, prm=None, pair=None, product=None):
    """host twins -> merge -> choose -> the three arrays as tuples"""
    lists = _lists(records[home], rows, targets, prm, pair)
    total = None
    for k, record in enumerate(records):
        one = _verdicts(record, lists, int(k == home), pair, product)
        total = one if total is None else ribbit_amd.primer_verdicts_merge(total, one)
    assert (total["records"] == len(records)).all() and (total["home_records"] == 1).all()
    return tuple(ps.as_tuples(a) for a in ribbit_amd.primer_shortlists_choose(lists, total, _params(None, pair)[1]))


def _contract(records, home, rows, targets, prm=None, pair=None, product=None, loops=False):
    return pg.genome_specific_primer_pairs(records, home, rows, targets, pc.params(**(prm or {})), pp.pair_params(**(pair or {})), pq.params(**(product or {})), loops=loops)


def _same(got, want, what):
    for g, w, fields in zip(got, want, (pp.FIELDS, pq.FIELDS, ps.FIELDS)):
        assert len(g) == len(w), what
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (what, i, [(f, x, y) for f, x, y in zip(fields, a, b) if x != y])


def test_the_three_pinned_genomes():
    genomes = pg.pinned_genomes()
    assert list(genomes) == list(pg.PINNED) and len(genomes) == 3
    for name, (home, other) in genomes.items():
        want = _contract([home, other], 0, [], [pg.TARGET], loops=True)
        assert want == _contract([home, other], 0, [], [pg.TARGET], loops=False), name
        (p,), (q,), (s,) = want
        assert (s[:6], (p[0], p[1], p[6], p[7])) == pg.PINNED[name], name
        assert s[1] == s[2] + s[3] + s[4] == p[30] and s[6:] == (0, 0)
        _same(_genome([home, other], 0, [], [pg.TARGET]), want, name)
        # either record first: home is a matter of position, and the sum does not depend on the order
        swapped = _contract([other, home], 1, [], [pg.TARGET])
        assert swapped == want, name
        _same(_genome([other, home.lower()], 1, [], [pg.TARGET]), want, name)
    # a copy in another record cannot form a product with the original: within one record the same constructions give 18 and 2
    assert ps.PINNED["best pair copied"][0][4:] == (18, 2) and pg.PINNED["best pair copied to the other record"][0][4:] == (14, 1)


def test_the_fixture_holds_the_pinned_genomes():
    """tests/golden/primer_genome_pinned.fa, which tools/probes/primer_genome_host_check.cpp reads: the home record and the three
    forms of the other one, as the contract module builds them"""
    genomes = list(pg.pinned_genomes().values())
    want = [("home", genomes[0][0])] + list(zip(("other", "other_with_best_pair", "other_with_both_flanks"), (g[1] for g in genomes)))
    assert [(name, bases) for name, bases, _ in ribbit_amd.read_fasta(os.path.join(ROOT, "tests", "golden", "primer_genome_pinned.fa"))] == want


def test_the_lists_and_verdicts_are_the_contracts():
    home, other = pg.pinned_genomes()["best pair copied to the other record"]
    targets = [pg.TARGET, (0, 30), (3990, 4000), (700, 730)]
    for prm, pair in (({}, {}), (dict(flank=60), dict(shortlist=3))):
        by_contract = pg.target_shortlists(home, [(650, 690)], targets, pc.params(**prm), pp.pair_params(**pair))
        lists = _lists(home, [(650, 690)], targets, prm, pair)
        assert lists.view("<i4").reshape(len(targets), 100).tolist() == [list(t) for t in pg.shortlists_as_tuples(home, by_contract)]
        for record, is_home in ((home, True), (other, False), (home, False)):
            letters = pq.letters_of(record)
            want = [pg.record_verdicts(letters, left, right, is_home, pp.pair_params(**pair)) for left, right, _ in by_contract]
            assert _verdict_tuples(_verdicts(record, lists, int(is_home), pair)) == want
    assert any(len(left) < 8 or len(right) < 8 for left, right, _ in by_contract) and any(len(left) == 0 for left, _, _ in by_contract)


def test_one_record_is_the_specific_contract():
    for name, (record, fields) in ps.constructed().items():
        want = ribbit_amd.host_record_specific_primer_pairs(record, [], [ps.TARGET], product_params=ribbit_amd.product_params(**fields))
        _same(_genome([record], 0, [], [ps.TARGET], product=fields), tuple(ps.as_tuples(a) for a in want), name)
    rs = np.random.RandomState(7)
    chosen = passed_over = 0
    for case in range(6):
        length = int(rs.randint(300, 3001))
        seq = pc.random_record(length, 50 + case, MOSTLY_BASES if case else pc.ALPHABET)
        if case % 2 == 0:
            seq = (seq[:length // 2] + seq[:length // 2])[:length]
        rows = pc.random_targets(length, rs, 4, longest=40).tolist()
        targets = pc.edge_targets(length) + pc.random_targets(length, rs, 6, longest=60).tolist()
        prm = dict(flank=int(rs.choice([0, 30, 200, 1000])), gc_clamp=int(rs.randint(2)), tm_min=520, tm_max=660) if rs.randint(2) else {}
        pair = dict(shortlist=int(rs.randint(1, 9))) if rs.randint(2) else dict(pp.LOOSE, shortlist=int(rs.randint(1, 9)))
        product = dict(seed=int(rs.randint(6, 16)), max_mismatches=int(rs.choice([0, 2, 32])), max_product=int(rs.choice([300, 4000, 2**31 - 1])),
                       max_sites=int(rs.choice([1, 2, 64])))
        if pc.params(**prm)["min_length"] < product["seed"]:
            product["seed"] = 15
        want = tuple(ps.as_tuples(a) for a in ribbit_amd.host_record_specific_primer_pairs(seq, rows, targets, *_params(prm, pair, product)))
        _same(_genome([seq], 0, rows, targets, prm, pair, product), want, (case, prm, pair, product))
        chosen += sum(s[0] >= 0 for s in want[2])
        passed_over += sum(s[0] != 0 and s[1] > 0 for s in want[2])
    assert chosen > 0 and passed_over > 0, (chosen, passed_over)


def test_a_genome_is_its_concatenation():
    """the records joined by max_product N, each target's home first: a spacer holds no site and is too long for a product to span,
    so the one-record answer is the genome's, as long as no list of the joined record is longer than max_sites (max_sites holds per
    record, so only then can the two differ)"""
    a, b, c = pg.pinned_genomes()["undisturbed"][0], pg.pinned_genomes()["best pair copied to the other record"][1], pg.pinned_genomes()["both flanks copied to the other record"][1]
    spacer = b"N" * pq.DEFAULTS["max_product"]
    targets = [pg.TARGET, (700, 730), (3000, 3040)]
    met = set()
    for records in ([a, b], [a, c], [a, b, c], [a, c, b], [b, a], [c, b, a]):
        home, others = records[0], records[1:]
        rows = [(690, 740)]
        want = tuple(ps.as_tuples(x) for x in ribbit_amd.host_record_specific_primer_pairs(spacer.join([home] + others), rows, targets))
        assert all(s[3] == 0 for s in want[2])
        for at in range(len(records)):      # the home record at every position of the input
            order = others[:at] + [home] + others[at:]
            _same(_genome(order, at, rows, targets), want, (len(records), at))
        met |= {("none" if s[0] < 0 else "first" if s[0] == 0 else "later") for s in want[2]}
    assert met == {"none", "first", "later"}


def _tiled_foreign_record(copies: int) -> bytes:
    """4,000 other bases with the left primer of the undisturbed record's best pair `copies` times, 40 bases from start to start"""
    home = ps.base_record()
    best = pp.record_primer_pairs(home, [], [pg.TARGET])[0]
    left = home[best[0]:best[0] + best[1]]
    record = pg.other_record()
    for j in range(copies):
        record = ps._put(record, 100 + 40 * j, left)
    return record


@pytest.mark.parametrize("copies,max_sites", [(2, 1), (70, 64)])
def test_max_sites_holds_per_record(copies, max_sites):
    home, foreign = ps.base_record(), _tiled_foreign_record(copies)
    product = dict(max_sites=max_sites)
    want = _contract([home, foreign], 0, [], [pg.TARGET], product=product)
    _same(_genome([home, foreign], 0, [], [pg.TARGET], product=product), want, (copies, max_sites))
    (s,) = want[2]
    assert s[3] > 0 and s[5] == -1      # the best pair's left primer: over, in the foreign record alone
    lists = _lists(home, [], [pg.TARGET])
    at_home, abroad = _verdicts(home, lists, 1, product=product), _verdicts(foreign, lists, 0, product=product)
    assert at_home["over"][0] == 0 and abroad["over"][0] != 0 and abroad["forward"][0].max() == copies
    # one more site than the longest kept list, summed over two records in which no list is too long, is not over
    half = _tiled_foreign_record(max_sites)
    total = ribbit_amd.primer_verdicts_merge(ribbit_amd.primer_verdicts_merge(at_home, _verdicts(half, lists, 0, product=product)), _verdicts(half, lists, 0, product=product))
    assert total["over"][0] == 0 and total["forward"][0].max() == 2 * max_sites + 1 > max_sites


def test_the_home_record_judged_as_foreign():
    record, _ = ps.constructed()["best pair copied"]
    lists = _lists(record, [], [ps.TARGET, (700, 730)])
    as_home, as_foreign = _verdicts(record, lists, 1), _verdicts(record, lists, 0)
    assert (as_home["own"] != 0).any() and (as_foreign["own"] == 0).all()
    assert (as_foreign["other"] == as_home["other"] | as_home["own"]).all() and (as_foreign["over"] == as_home["over"]).all()
    assert (as_foreign["admissible"] == as_home["admissible"]).all() and (as_foreign["home_records"] == 0).all()


def test_the_sum_is_associative_and_commutative():
    home, b = pg.pinned_genomes()["best pair copied to the other record"]
    c = _tiled_foreign_record(70)
    lists = _lists(home, [], [pg.TARGET, (700, 730)])
    x, y, z = _verdicts(home, lists, 1), _verdicts(b, lists, 0), _verdicts(c, lists, 0)
    m = ribbit_amd.primer_verdicts_merge
    assert m(x, y).tobytes() == m(y, x).tobytes() and m(m(x, y), z).tobytes() == m(x, m(y, z)).tobytes() == m(m(z, x), y).tobytes()
    assert m(x, y)["first_others"].tolist() != m(m(x, y), z)["first_others"].tolist() and -1 in m(m(x, y), z)["first_others"].tolist()
    # the counts saturate
    big = x.copy()
    big["forward"][:] = 2**31 - 2
    big["records"][:] = 2**31 - 1
    assert (m(big, big)["forward"] == 2**31 - 1).all() and (m(big, x)["records"] == 2**31 - 1).all()
    assert len(m(x[:0], y[:0])) == 0


def test_what_merge_and_choose_refuse():
    home, other = pg.pinned_genomes()["undisturbed"]
    lists = _lists(home, [], [pg.TARGET, (700, 730)])
    x, y = _verdicts(home, lists, 1), _verdicts(other, lists, 0)
    bad = y.copy()
    bad["admissible"][1] ^= 1
    with pytest.raises(ribbit_amd.RibbitHipError, match="ribbit_primer_verdicts_merge error -1: target 1: the two verdicts are of different admissible pairs"):
        ribbit_amd.primer_verdicts_merge(x, bad)
    with pytest.raises(ValueError, match="2 and 1 verdicts"):
        ribbit_amd.primer_verdicts_merge(x, y[:1])
    label = "ribbit_primer_shortlists_choose error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 0: judged on 0 home records, not 1"):
        ribbit_amd.primer_shortlists_choose(lists, y)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 0: judged on 2 home records, not 1"):
        ribbit_amd.primer_shortlists_choose(lists, ribbit_amd.primer_verdicts_merge(x, x))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 1: the verdicts are not of these lists' admissible pairs"):
        wrong = x.copy()
        wrong["admissible"][1] ^= 1
        ribbit_amd.primer_shortlists_choose(lists, wrong)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "shortlist 0 is outside 1 .. 8"):
        ribbit_amd.primer_shortlists_choose(lists, x, ribbit_amd.primer_pair_params(shortlist=0))
    with pytest.raises(ValueError, match="2 lists and 1 verdicts"):
        ribbit_amd.primer_shortlists_choose(lists, x[:1])
    assert all(len(a) == 0 for a in ribbit_amd.primer_shortlists_choose(lists[:0], x[:0]))
    L = ribbit_amd.load_library()
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    q = ribbit_amd.primer_pair_params()
    good = [lists.ctypes.data, x.ctypes.data, 2, C.byref(q), C.byref(a), C.byref(b), C.byref(c)]
    for k in (0, 1, 3, 4, 5, 6):
        assert L.ribbit_primer_shortlists_choose(*(None if j == k else v for j, v in enumerate(good))) == -1 and b"null argument" in L.ribbit_hip_last_error(), k
    assert L.ribbit_primer_verdicts_merge(None, x.ctypes.data, 2) == -1 and L.ribbit_primer_verdicts_merge(x.ctypes.data, None, 2) == -1
    assert L.ribbit_primer_verdicts_merge(None, None, 0) == 0


def test_every_refusal_of_the_twins_and_the_empty_cases():
    home, other = pg.pinned_genomes()["undisturbed"]
    label = "ribbit_host_record_primer_shortlists error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "flank 1001 is outside 0 .. 1000"):
        _lists(home, [], [pg.TARGET], dict(flank=1001))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "shortlist 9 is outside 1 .. 8"):
        _lists(home, [], [pg.TARGET], None, dict(shortlist=9))
    with pytest.raises(TypeError, match="pair_params: a PrimerPairParams"):
        ribbit_amd.host_record_primer_shortlists(home, [], [pg.TARGET], None, pp.PAIR_DEFAULTS)
    lists = _lists(home, [], [pg.TARGET, (700, 730)])
    label = "ribbit_host_record_shortlist_verdicts error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "max_pair_end 33 is outside 0 .. 32"):
        _verdicts(other, lists, 0, dict(max_pair_end=33))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "max_sites 1025 is outside 1 .. 1024"):
        _verdicts(other, lists, 0, None, dict(max_sites=1025))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "seed 5 is outside 6 .. 16"):
        _verdicts(other, lists, 0, None, dict(seed=5))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "home 2 is neither 0 nor 1"):
        _verdicts(other, lists, 2)
    with pytest.raises(TypeError, match="product_params: a ProductParams"):
        ribbit_amd.host_record_shortlist_verdicts(other, lists, 0, None, pq.DEFAULTS)
    # malformed lists, each with the target's index
    gap = lists.copy()
    gap["left"][1][2] = (-1, 0, 0, 0, 0, 0)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 1: a held place behind an empty one"):
        _verdicts(other, gap, 0)
    short = lists.copy()
    short["right"]["length"][0][0] = 14
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 0: a primer of 14 bases, not 15 .. 32"):
        _verdicts(other, short, 0)
    assert len(_verdicts(other, short, 0, None, dict(seed=14))) == 2
    long = lists.copy()
    long["left"]["length"][1][7] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 1: a primer of 33 bases, not 15 .. 32"):
        _verdicts(other, long, 0)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "target 0: 8 held places, more than shortlist 3"):
        _verdicts(other, lists, 0, dict(shortlist=3))
    with pytest.raises(ribbit_amd.RibbitHipError, match="ribbit_primer_shortlists_choose error -1: target 1: a held place behind an empty one"):
        ribbit_amd.primer_shortlists_choose(gap, _verdicts(home, lists, 1))
    # no targets, records without a base, without a site, shorter than a primer
    assert len(_lists(home, [], [])) == 0 and len(_verdicts(other, lists[:0], 0)) == 0
    empty = _lists(b"", [], [(0, 5)])
    assert empty.view("<i4").tolist() == list(pc.NO_PRIMER * 16 + (0, 0, 0, 0))
    assert _verdict_tuples(_verdicts(other, empty, 1)) == [(0, 0, 0, 0, (0,) * 16, (0,) * 16, 0, 1, 1, 0)]
    for nothing in (b"", b"ACGTACGTAC", b"N" * 300):
        v = _verdicts(nothing, lists, 0)
        assert (v["admissible"] == _verdicts(home, lists, 1)["admissible"]).all() and v["admissible"][0] != 0
        assert not (v["over"] | v["other"] | v["own"]).any() and not v["forward"].any() and not v["reverse"].any() and (v["first_others"] == 0).all()
    L = ribbit_amd.load_library()
    out = C.c_void_p()
    p, q, r = _params()
    tg = np.array([pg.TARGET], np.int32)
    good = [home, len(home), None, 0, tg.ctypes.data, 1, C.byref(p), C.byref(q), C.byref(out)]
    f = L.ribbit_host_record_primer_shortlists
    for k in (4, 6, 7, 8):
        assert f(*(None if j == k else v for j, v in enumerate(good))) == -1 and b"null argument" in L.ribbit_hip_last_error(), k
    assert f(None, 5, *good[2:]) == -1 and b"bad sequence" in L.ribbit_hip_last_error()
    assert f(home, -1, *good[2:]) == -1 and b"a record of -1 bases" in L.ribbit_hip_last_error()
    good = [other, len(other), lists.ctypes.data, 2, 0, C.byref(q), C.byref(r), C.byref(out)]
    f = L.ribbit_host_record_shortlist_verdicts
    for k in (2, 5, 6, 7):
        assert f(*(None if j == k else v for j, v in enumerate(good))) == -1 and b"null argument" in L.ribbit_hip_last_error(), k
    assert f(None, 5, *good[2:]) == -1 and b"bad sequence" in L.ribbit_hip_last_error()
    assert L.ribbit_hip_record_primer_shortlists(None, None, 0, tg.ctypes.data, 1, C.byref(p), C.byref(q), C.byref(out)) == -1 and b"null handle" in L.ribbit_hip_last_error()
    assert L.ribbit_hip_record_shortlist_verdicts(None, *good[2:]) == -1 and b"null handle" in L.ribbit_hip_last_error()


def test_names_sizes_and_the_binding():
    for name in ("PRIMER_SHORTLISTS_DT", "PRIMER_VERDICTS_DT", "host_record_primer_shortlists", "host_record_shortlist_verdicts", "primer_verdicts_merge",
                 "primer_shortlists_choose"):
        assert name in ribbit_amd.__all__ and hasattr(ribbit_amd, name)
    assert ribbit_amd.PRIMER_SHORTLISTS_DT.itemsize == 400 and ribbit_amd.PRIMER_VERDICTS_DT.itemsize == 176
    assert ribbit_amd.PRIMER_VERDICTS_DT.names == pg.VERDICT_FIELDS
    assert hasattr(ribbit_amd.Scanner, "record_primer_shortlists") and hasattr(ribbit_amd.Scanner, "record_shortlist_verdicts")
    for symbol in ("ribbit_hip_record_primer_shortlists", "ribbit_hip_record_shortlist_verdicts", "ribbit_host_record_primer_shortlists",
                   "ribbit_host_record_shortlist_verdicts", "ribbit_primer_verdicts_merge", "ribbit_primer_shortlists_choose", "ribbit_primer_genome_free"):
        assert symbol in ribbit_amd.ABI_SYMBOLS
    assert ribbit_amd.load_library().ribbit_hip_abi_version() == 1


# ---- the command-line tool, up to the GPU
def _fails(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == message, args


def _dies(args, message):
    _fails(args, "ribbit-hip: " + message + "\n")


@needs_tool
def test_cli_the_qualifier_needs_its_output(tmp_path):
    _dies(["--primer-genome-flank", "5"], "--primer-genome-flank needs --primer-genome-bed")
    _dies(["-i", "in.fa", "--primer-genome-flank=5"], "--primer-genome-flank needs --primer-genome-bed")
    _dies(["--primer-genome-flank", "5", "--primer-specific-bed", "b"], "--primer-genome-flank needs --primer-genome-bed")
    _dies(["--primer-specific-flank", "5", "--primer-genome-bed", "b"], "--primer-specific-flank needs --primer-specific-bed")
    # the first in the order of the outputs
    _dies(["--primer-genome-flank", "5", "--primer-specific-flank", "5"], "--primer-specific-flank needs --primer-specific-bed")
    _fails(["--primer-genome-bed", tmp_path / "missing" / "out", "--primer-genome-flank", "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values_and_file_names(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("1001", "-1", "x", "10000", "1e3", "", "+5"):
        _dies(["-i", "in.fa", "--primer-genome-bed", "b", "--primer-genome-flank", value],
              f"--primer-genome-flank wants a whole number of bases (0 .. 1000), got '{value}'")
    for value in ("0", "1000", "0200"):
        _dies(["-i", tmp_path / "in.fa", "--primer-genome-bed", out, "--primer-genome-flank", value], f"--primer-genome-bed: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--primer-genome-bed", "b", "--primer-genome-flank"], "the required argument for option '--primer-genome-flank' is missing")
    _dies(["--primer-genome-bed="], "--primer-genome-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-genome-bed", ""], "--primer-genome-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-genome-bed"], "the required argument for option '--primer-genome-bed' is missing")
    for option in ("--primer-genome-seed", "--primer-genome-max-sites", "--primer-genomes-bed", "--primer-genome-background"):
        _dies(["-i", "in.fa", "--primer-genome-bed", "x", option, "3"], f"unrecognised option '{option}'")


@needs_tool
def test_cli_the_file_is_opened_last_of_21(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    options = EARLIER_OUTPUTS + ["--primer-genome-bed"]
    assert len(options) == 21
    for bad in (19, 20):
        d = tmp_path / f"bad{bad}"
        d.mkdir()
        paths = [d / "missing" / "out" if k == bad else d / f"out{k}" for k in range(len(options))]
        args = ["-i", tmp_path / "in.fa", "--overlap-with", other]
        for k in reversed(range(len(options))):
            args += [options[k], paths[k]]
        _dies(args, f"{options[bad]}: cannot open '{paths[bad]}' for writing")
        assert [p.exists() for p in paths] == [k < bad for k in range(len(options))]


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    names = ["--primer-specific-bed", "--primer-specific-flank", "--primer-genome-bed", "--primer-genome-flank"]
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[1]:at[2]].endswith("Default: 200") and r.stderr[at[3]:].rstrip("\n").endswith("Default: 200")
    assert r.stderr[at[3]:].count("\n  --") == 1      # the last entry of the help
    entry = " ".join(r.stderr[at[2]:at[3]].split())
    assert "ALL records of the input" in entry and "there is no fallback" in entry and "read a second time" in entry and "600 bytes per row" in entry
    # --primer-specific-bed's entry stays as it was
    assert "Only the record itself is searched, not the other records of the input" in " ".join(r.stderr[at[0]:at[1]].split())
