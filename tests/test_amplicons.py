"""Every chosen primer pair typed on another record, without a GPU: ribbit_host_record_pair_amplicons against the plain statement of
the contract (tests/amplicons_contract.py) on the pinned values and on constructed records, the sum over records, the marker text,
every refusal, and ribbit-hip's two options up to the GPU."""
import os
import subprocess

import numpy as np
import pytest

import amplicons_contract as ac
import primer_pairs_contract as pp
import primer_products_contract as prc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
DT = ribbit_amd.PAIR_AMPLICONS_DT
PAIR = prc.pair_tuple(ac.A, ac.B, 0, 0)      # (only the primers' length and bases are read)
NO_PAIR = (-1, 0, 0, 0, 0, 0) * 2 + (0,) * 20


def _twin(record, pairs, motifs, label=0, **fields):
    got = ribbit_amd.host_record_pair_amplicons(record if isinstance(record, bytes) else record.encode(), np.array(pairs, dtype=ribbit_amd.PRIMER_PAIRS_DT), motifs, label,
                                                ribbit_amd.product_params(**fields))
    assert got.dtype == DT and DT.names == ac.FIELDS and DT.itemsize == 64
    return ac.as_tuples(got)


def _contract(record, pairs, motifs, label=0, **fields):
    return ac.record_pair_amplicons(record if isinstance(record, bytes) else record.encode(), pairs, motifs, label, prc.params(**fields))


def _both(record, motif, label=0, **fields):
    got = _twin(record, [PAIR], [motif], label, **fields)
    assert got == _contract(record, [PAIR], [motif], label, **fields), (record[:80], motif, fields)
    return got[0]


def test_the_pinned_values():
    assert len(ac.REC) == 76 and len(ac.PINNED) == 11
    for (record, motif), value in ac.PINNED.items():
        assert _both(record, motif, 3) == ac.pinned_fields(value, 3), (record, motif)


def _rotation(w, rs):
    k = rs.randint(len(w))
    return w[k:] + w[:k]


def constructed_body(motif, rs, pieces=5):
    """rotations of the motif and of its reverse complement, repeated and cut at any length, 0 .. 4 random letters between them"""
    body = ""
    for _ in range(pieces):
        w = _rotation(motif if rs.randint(2) else pp.reverse_complement(motif), rs)
        body += (w * 8)[:rs.randint(1, 5 * len(w) + 2)]
        body += "".join(rs.choice(list("ACGTN"), rs.randint(5)))
    return body


def random_motif(m, rs):
    return "".join(rs.choice(list("ACGT"), m))


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6, 7, 31, 32, 33, 64, 65, 100])
def test_constructed_records_equal_the_contract(m):
    rs = np.random.RandomState(100 + m)
    tracts = strands = 0
    for _ in range(8):
        motif = random_motif(m, rs)
        record = ac.LP + constructed_body(motif, rs) + ac.RP
        if rs.randint(3) == 0:
            record = record.lower()
        a = _both(record, motif, max_product=100000)
        assert a[:6] == (1, 0, 0, 1, 1, 0) and a[6:12] == (0, len(record), 0, 1, 18, len(record) - 18)
        tracts += a[12] >= 0
        strands += a[14]
    assert tracts >= 4 and (m == 1 or 0 < strands)      # (both strands are met; a homopolymer's other strand is met by chance only)


def test_inner_parts_at_their_limits():
    # an empty inner part; a tract that is the whole inner part and ends where the right primer starts, in a product that ends at the
    # record's last base; one unit short of a tract; exactly two units
    assert _both(ac.LP + ac.RP, "CA")[6:] == (0, 36, 0, 1, 18, 18, -1, -1, 0, 0)
    assert _both(ac.LP + "CA" * 9 + ac.RP, "AC")[6:] == (0, 54, 0, 1, 18, 36, 18, 36, 0, 0)
    assert _both(ac.LP + "TCAT" + ac.RP, "CA")[12:15] == (-1, -1, 0)
    assert _both(ac.LP + "TCACAT" + ac.RP, "CA")[12:15] == (19, 23, 0)
    assert _both(ac.LP + "TCACT" + ac.RP, "CA")[12:15] == (-1, -1, 0)
    # equal lengths: the leftmost; a motif that is its own reverse complement: strand 0
    assert _both(ac.LP + "CACACATTTGTGTGA" + ac.RP, "CA")[12:15] == (18, 24, 0)
    assert _both(ac.LP + "TGTGTGAAGCACACAT" + ac.RP, "CA")[12:15] == (18, 24, 1)
    assert _both(ac.LP + "GATATATATC" + ac.RP, "AT")[12:15] == (19, 27, 0)
    # the record in lower case and with other bytes
    assert _both((ac.LP + "CACAnCACACA" + ac.RP).lower(), "CA")[12:15] == (23, 29, 0)


def test_over_left_left_and_two_products_with_one_start():
    twice = ac.REC + "ACGTAGCTAGCTAGGATCGA" + ac.REC
    assert _both(twice, "CA", max_sites=1) == (2, 0, 0, 2, -1) + ac.NONE
    assert _both(twice, "CA", max_sites=2)[4] == 3
    # the left primer against itself, nearer than the right primer: orientation l
    left_left = ac.LP + "CACACACA" + pp.reverse_complement(ac.LP) + ac.Y + ac.RP
    assert _both(left_left, "CA") == (1, 1, 0, 1, 2, 0, 0, 44, 0, 0, 18, 26, 18, 26, 0, 0)
    # the right primer as both ends: orientation r
    right_right = pp.reverse_complement(ac.RP) + "TGTGTGTG" + ac.RP
    assert _both(right_right, "CA") == (0, 0, 1, 1, 1, 0, 0, 44, 1, 1, 18, 26, 18, 26, 1, 0)
    # two products from one forward site: the nearer end is the first
    two = ac.LP + ac.X + ac.RP + "GAGAGAGA" + ac.RP
    assert _both(two, "GA")[4:12] == (2, 0, 0, 46, 0, 1, 18, 28)
    # a == b: a site of a and a site of b at one place, the first product is a's with a's
    same = prc.pair_tuple(prc.PALINDROME, prc.PALINDROME, 0, 0)
    record = prc.PALINDROME + prc.PALINDROME
    got = _twin(record, [same], ["ACGT"])
    assert got == _contract(record, [same], ["ACGT"]) and got[0][4:12] == (4, 0, 0, 32, 0, 0, 16, 16)
    # a max_product that leaves only the far pairing out
    assert _both(two, "GA", max_product=46)[4] == 1 and _both(two, "GA", max_product=45)[4] == 0


def test_rows_without_a_pair_and_empty_records():
    record = ac.REC.encode()
    got = _twin(record, [NO_PAIR, PAIR, NO_PAIR], ["CA", "CA", "ACGT"], 7)
    assert got == _contract(record, [NO_PAIR, PAIR, NO_PAIR], ["CA", "CA", "ACGT"], 7)
    assert got[0] == got[2] == ac.NO_PAIR and got[1][5] == 7
    assert _twin(b"", [PAIR, NO_PAIR], ["CA", "CA"]) == [(0, 0, 0, 0, 0) + ac.NONE, ac.NO_PAIR]
    assert _twin(b"N" * 700, [PAIR], ["CA"]) == [(0, 0, 0, 0, 0) + ac.NONE]
    assert len(_twin(record, np.zeros(0, ribbit_amd.PRIMER_PAIRS_DT), [])) == 0
    # a pool and its offsets as bed_motifs hands them out
    pool, offsets = ribbit_amd.bed_motifs("r\t0\t9\tCA\t.\t.\t4\t.\t.\t.\t9M\nr\t0\t9\tTG\t.\t.\t4\t.\t.\t.\t9M\n")
    assert _twin(record, [PAIR, PAIR], (pool, offsets)) == _contract(record, [PAIR, PAIR], ["CA", "TG"])


def _arr(rows):
    return np.array(rows, dtype=DT)


def test_the_laws_of_the_sum():
    first = _twin(ac.REC, [PAIR], ["CA"], 0)[0]
    longer = _twin(ac.LP + ac.X + "CA" * 17 + ac.Y + ac.RP, [PAIR], ["CA"], 1)[0]
    none = _twin(ac.LP + ac.X, [PAIR], ["CA"], 2)[0]
    over = _twin(ac.REC + "ACGT" + ac.REC, [PAIR], ["CA"], 3, max_sites=1)[0]
    merge = lambda a, b: ac.as_tuples(ribbit_amd.pair_amplicons_merge(_arr([a]), _arr([b])))[0]
    for a in (first, longer, none, over, ac.NO_PAIR):
        for b in (first, longer, none, over, ac.NO_PAIR):
            assert merge(a, b) == ac.merge(a, b), (a, b)
    # the first record's product is kept, whichever record comes later; a record without a product does not hide it
    assert merge(first, longer)[4:] == (2,) + first[5:] and merge(longer, first)[4:] == (2,) + longer[5:]
    assert merge(none, longer) == (2, 0, 0, 1, 1) + longer[5:] and merge(longer, none) == (2, 0, 0, 1, 1) + longer[5:]
    # -1 wins, and takes the product with it
    assert merge(first, over) == (3, 0, 0, 3, -1) + ac.NONE == merge(over, first)
    # the counts and products saturate
    big = (ac.INT32_MAX - 1, 5, 0, ac.INT32_MAX, ac.INT32_MAX - 2) + first[5:]
    assert merge(big, (3, 1, 0, 1, 7) + longer[5:]) == (ac.INT32_MAX, 6, 0, ac.INT32_MAX, ac.INT32_MAX) + first[5:]
    # in record order over a genome, as the contract sums it
    genome = [(ac.LP + ac.X).encode(), (ac.LP + ac.X + "CA" * 17 + ac.Y + ac.RP).encode(), ac.REC.encode()]
    total = None
    for k, bases in enumerate(genome):
        here = ribbit_amd.host_record_pair_amplicons(bases, np.array([PAIR, NO_PAIR], dtype=ribbit_amd.PRIMER_PAIRS_DT), ["CA", "CA"], k)
        total = here if total is None else ribbit_amd.pair_amplicons_merge(total, here)
    assert ac.as_tuples(total) == ac.genome_amplicons(genome, [PAIR, NO_PAIR], ["CA", "CA"]) and ac.as_tuples(total)[0][4:8] == (2, 1, 0, 90)
    with pytest.raises(ValueError, match="1 and 2 amplicons"):
        ribbit_amd.pair_amplicons_merge(_arr([first]), _arr([first, first]))


def test_every_refusal_of_the_twin():
    label = "ribbit_host_record_pair_amplicons error -1: "
    pairs = np.array([PAIR], dtype=ribbit_amd.PRIMER_PAIRS_DT)
    call = lambda motifs, record=0, pairs=pairs, **fields: ribbit_amd.host_record_pair_amplicons(ac.REC.encode(), pairs, motifs, record, ribbit_amd.product_params(**fields))
    for fields, message in ((dict(seed=5), "seed 5 is outside 6 .. 16"), (dict(seed=17), "seed 17 is outside 6 .. 16"),
                            (dict(max_mismatches=-1), "max_mismatches -1 is outside 0 .. 32"), (dict(max_mismatches=33), "max_mismatches 33 is outside 0 .. 32"),
                            (dict(max_product=0), "max_product 0 is below 1"), (dict(max_sites=0), "max_sites 0 is outside 1 .. 1024"),
                            (dict(max_sites=1025), "max_sites 1025 is outside 1 .. 1024")):
        with pytest.raises(ribbit_amd.RibbitHipError, match=label + message):
            call(["CA"], **fields)
    short = np.array([NO_PAIR, prc.pair_tuple("GATTACAGATTACA", ac.B, 0, 0)], dtype=ribbit_amd.PRIMER_PAIRS_DT)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 1: a primer of 14 bases, not seed 15 .. 32"):
        call(["CA", "CA"], pairs=short)
    assert len(call(["CA", "CA"], pairs=short, seed=14)) == 2
    long = pairs.copy()
    long["right_length"] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 0: a primer of 33 bases, not seed 15 .. 32"):
        call(["CA"], pairs=long)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "record -1 is below 0"):
        call(["CA"], record=-1)
    for motifs, message in (([""], "row 0: an empty motif"), (["A" * 1024], r"row 0: a motif of 1024 bytes \(at most 1023\)"), (["CAN"], "row 0: a motif with a byte outside ACGT"),
                            (["ca"], "row 0: a motif with a byte outside ACGT"), ((b"CA", [1, 2]), "the motifs' offsets start at 1, not at 0"),
                            ((b"CA", [0, -1]), "row 0: the motifs' offsets do not ascend")):
        with pytest.raises(ribbit_amd.RibbitHipError, match=label + message):
            call(motifs)
    assert len(call(["A" * 1023])) == 1
    # a row without a pair still has its motif checked, as ribbit_hip_record_classes checks every row's
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "row 0: an empty motif"):
        call(["", "CA"], pairs=short, seed=14)
    with pytest.raises(ValueError, match="1 pairs want 2 offsets"):
        call(["CA", "CA"])
    with pytest.raises(ValueError, match="record 4294967296 is not an int32"):
        call(["CA"], record=1 << 32)
    with pytest.raises(TypeError):
        ribbit_amd.host_record_pair_amplicons(ac.REC.encode(), pairs, ["CA"], 0, ribbit_amd.primer_params())


BED = "".join(f"home\t{100 * k}\t{100 * k + 20}\t{m}\t.\t.\t10\t.\t.\t.\t20M\n" for k, m in enumerate(("CA", "CA", "CA", "CA", "GATA", "CA")))


def test_the_text_for_none_one_two_over_and_no_pair():
    designed = list(PAIR)
    designed[0], designed[6], designed[14] = 5, 63, 76      # where the pair lies at home, and its designed product
    designed = tuple(designed)
    one = _twin(ac.LP + ac.X + "CA" * 17 + ac.Y + ac.RP, [designed], ["CA"], 1)[0]
    reversed_one = _twin(pp.reverse_complement(ac.REC), [designed], ["CA"], 0)[0]
    none = _twin(ac.LP + ac.X, [designed], ["CA"], 0)[0]
    two = _twin(ac.REC + "ACGT" + ac.REC, [designed], ["CA"], 1)[0]
    over = _twin(ac.REC + "ACGT" + ac.REC, [designed], ["CA"], 1, max_sites=1)[0]
    no_tract = _twin(ac.LP + "GATAGAT" + ac.RP, [designed], ["GATA"], 2)[0]
    pairs = [designed, designed, designed, designed, designed, NO_PAIR]
    amplicons = [one, none, two, over, no_tract, ac.NO_PAIR]
    names = ["first", "second one", "third"]
    got = ribbit_amd.bed_marker_text(BED, np.array(pairs, dtype=ribbit_amd.PRIMER_PAIRS_DT), _arr(amplicons), names).decode()
    assert got == ac.marker_lines(BED, pairs, amplicons, names)
    lines = [l.split("\t") for l in got.splitlines()]
    assert all(len(l) == 31 for l in lines) and "".join("\t".join(l[:11]) + "\n" for l in lines) == BED
    assert lines[0][11:20] == ["5", "23", ac.LP, "0.0", "63", "81", ac.B, "0.0", "76"]
    assert lines[0][20:] == ["1", "second one", "0", "90", "+", "90", "14", "28", "63", "35", "17"]
    assert lines[1][20:] == ["0"] + ["."] * 10 and lines[2][20:] == ["3"] + ["."] * 10 and lines[3][20:] == ["."] * 11
    assert lines[4][20:] == ["1", "third", "0", "43", "+", "43", "-33", ".", ".", ".", "."]
    assert lines[5][11:] == ["."] * 20
    text = ribbit_amd.bed_marker_text(BED.splitlines()[0], [designed], _arr([reversed_one]), names).decode()
    assert text.rstrip("\n").split("\t")[20:] == ["1", "first", "0", "76", "-", "76", "0", "27", "48", "21", "10"]
    assert ribbit_amd.bed_marker_text("", [], _arr([]), []) == b""
    # what it refuses
    label = "ribbit_bed_marker_text error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "row 0: record 1 is none of the names"):
        ribbit_amd.bed_marker_text(BED.splitlines()[0], [designed], _arr([one]), ["only"])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "the BED text has 6 lines, not the 1 of the rows"):
        ribbit_amd.bed_marker_text(BED, [designed], _arr([one]), names)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "line 0 of the BED text is not a row"):
        ribbit_amd.bed_marker_text("home\t1\t2\n", [designed], _arr([one]), names)
    bad = list(designed)
    bad[1] = 40
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "row 0: a primer of 40 bases, not 1 .. 32"):
        ribbit_amd.bed_marker_text(BED.splitlines()[0], [tuple(bad)], _arr([one]), names)
    with pytest.raises(ValueError, match="1 pairs and 2 amplicons"):
        ribbit_amd.bed_marker_text(BED.splitlines()[0], [designed], _arr([one, one]), names)
    # a record that is not used is not looked up: two products name no record
    assert b"\t3" + b"\t." * 10 in ribbit_amd.bed_marker_text(BED.splitlines()[0], [designed], _arr([two]), ["only", "two"])


def test_names_sizes_and_the_binding():
    for name in ("PAIR_AMPLICONS_DT", "host_record_pair_amplicons", "pair_amplicons_merge", "bed_marker_text"):
        assert name in ribbit_amd.__all__ and hasattr(ribbit_amd, name)
    assert hasattr(ribbit_amd.Scanner, "record_pair_amplicons")
    for symbol in ("ribbit_hip_record_pair_amplicons", "ribbit_host_record_pair_amplicons", "ribbit_pair_amplicons_merge", "ribbit_pair_amplicons_free",
                   "ribbit_bed_marker_text"):
        assert symbol in ribbit_amd.ABI_SYMBOLS and hasattr(ribbit_amd.load_library(), symbol)
    assert ribbit_amd.load_library().ribbit_hip_abi_version() == 1


# ---- the tool up to the GPU
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_cli_each_option_needs_the_other(tmp_path):
    _dies(["-i", "in.fa", "--marker-fasta", "other.fa"], "--marker-fasta needs --marker-bed")
    _dies(["--marker-bed=markers.bed", "-i", "in.fa"], "--marker-bed needs --marker-fasta")
    _dies(["-i", "in.fa", "--marker-bed", "markers.bed", "--primer-genome-bed", "g.bed"], "--marker-bed needs --marker-fasta")
    _dies(["-i", "in.fa", "--marker-fasta", "", "--marker-bed", "m"], "--marker-fasta wants a file name")
    _dies(["-i", "in.fa", "--marker-fasta", "o.fa", "--marker-bed="], "--marker-bed wants a file name")
    _dies(["-i", "in.fa", "--marker-fasta"], "the required argument for option '--marker-fasta' is missing")
    # the qualifier of the selection still needs its own output
    _dies(["-i", "in.fa", "--marker-fasta", "o.fa", "--marker-bed", "m", "--primer-genome-flank", "50"], "--primer-genome-flank needs --primer-genome-bed")


@needs_tool
def test_cli_the_files_are_opened_before_the_gpu(tmp_path):
    other = tmp_path / "other.fa"
    other.write_text(">a\nACGT\n")
    _dies(["-i", "in.fa", "--marker-fasta", tmp_path / "missing.fa", "--marker-bed", tmp_path / "m.bed"],
          f"--marker-fasta: cannot open '{tmp_path / 'missing.fa'}' for reading")
    assert not (tmp_path / "m.bed").exists()
    _dies(["-i", "in.fa", "--marker-fasta", other, "--marker-bed", tmp_path / "missing" / "m.bed"],
          f"--marker-bed: cannot open '{tmp_path / 'missing' / 'm.bed'}' for writing")


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    at = [r.stderr.index(f"\n  {name} arg ") for name in ("--timing", "--marker-fasta", "--marker-bed", "--masked-fasta")]
    assert at == sorted(at)
    entry = " ".join(r.stderr[at[2]:at[3]].split())
    assert "20 columns" in entry and "--primer-genome-flank" in entry and "exactly one product" in entry and "whole units" in entry
