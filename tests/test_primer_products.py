"""In-silico PCR without a GPU: the pinned values of the contract through its plain statement (tests/primer_products_contract.py)
and through both host twins; ribbit_host_record_oligo_sites against that statement on random records; defaults and struct sizes;
every refusal with its text; the text byte for byte; with_random_background; and ribbit-hip's handling of --primer-product-bed and
--primer-product-flank up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import primer_pairs_contract as pp
import primer_products_contract as pq
import primers_contract as pc
import ribbit_amd
from ribbit_amd.simulate import simulate_sequence, with_random_background

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed", "--nearest-bed", "--nearest-other-bed", "--composition-bed",
                   "--composition-track", "--primer-bed", "--primer-pair-bed"]


def pair_row(a: str, b: str, left_start: int, right_start: int):
    """a hand-made PRIMER_PAIRS_DT record"""
    return np.array([pq.pair_tuple(a, b, left_start, right_start)], dtype=ribbit_amd.PRIMER_PAIRS_DT)


def test_the_pinned_values():
    assert len(pq.PINNED) >= 8
    for (record, a, b, left_start, right_start, fields), want in pq.PINNED.items():
        prm = pq.params(**dict(fields))
        assert pq.pair_products(record.encode(), a, b, left_start, right_start, prm) == want, (record, fields)
        for seq in (record.encode(), record.lower().encode()):
            got = ribbit_amd.host_record_primer_products(seq, pair_row(a, b, left_start, right_start), ribbit_amd.product_params(**dict(fields)))
            assert got.dtype == ribbit_amd.PRIMER_PRODUCTS_DT and got.dtype.names == pq.FIELDS and pq.as_tuples(got) == [want], (record, fields)
        # the four counts are the oligos' own
        sites, positions = ribbit_amd.host_record_oligo_sites(record.encode(), [a, b.lower()], ribbit_amd.product_params(**dict(fields)))
        assert tuple(sites["forward"]) + tuple(sites["reverse"]) == (want[0], want[2], want[1], want[3])
        assert pq.sites_as_lists(sites, positions) == pq.contract_sites(record.encode(), [a, b], prm)


def test_a_palindrome_has_both_sites_at_one_position():
    sites, positions = ribbit_amd.host_record_oligo_sites(b"TT" + pq.PALINDROME.encode() + b"GG", [pq.PALINDROME])
    assert pq.as_tuples(sites) == [(1, 1, 0, 1)] and positions.tolist() == [2, 2]


@pytest.mark.parametrize("seed", range(6))
def test_random_oligos_on_random_records(seed):
    """50 cases a seed, 300 in all: oligos cut from the record (either strand, a few bases changed) so that sites exist, on an alphabet
    with N, lower case and IUPAC letters; every parameter drawn"""
    rs = np.random.RandomState(100 + seed)
    found = 0
    for case in range(50):
        length = int(rs.choice([0, 5, 40, 200, 700]))
        # few distinct letters on the short records make sites that were not planted
        seq = pc.random_record(length, 1000 * seed + case, b"ACGT" * 30 + b"acgt" * 3 + b"NnRYx-" if case % 2 else b"AC" * 12 + b"GTacN")
        prm = pq.params(seed=int(rs.randint(6, 17)), max_mismatches=int(rs.choice([0, 1, 2, 5, 32])), max_sites=int(rs.choice([1, 2, 64, 1024])))
        oligos = []
        for _ in range(4):
            k = int(rs.randint(prm["seed"], 33))
            if length >= k and rs.randint(4):
                at = int(rs.randint(0, length - k + 1))
                letters = [ch if ch in "ACGT" else "ACGT"[rs.randint(4)] for ch in seq[at:at + k].decode().upper()]
                for _ in range(int(rs.randint(0, 3))):
                    letters[int(rs.randint(k))] = "ACGT"[rs.randint(4)]
                o = "".join(letters)
                oligos.append(pp.reverse_complement(o) if rs.randint(2) else o)
            else:
                oligos.append("".join("ACGT"[c] for c in rs.randint(0, 4, k)))
        sites, positions = ribbit_amd.host_record_oligo_sites(seq, oligos, ribbit_amd.product_params(**prm))
        got, want = pq.sites_as_lists(sites, positions), pq.contract_sites(seq, oligos, prm)
        assert got == want, (seed, case, prm, oligos)
        found += sum(r[0] + r[1] for r in want)
        # the first two as a pair, at the places of their first sites if they have any
        f, v = pq.oligo_sites(seq, oligos[0], prm["seed"], prm["max_mismatches"])[0], pq.oligo_sites(seq, oligos[1], prm["seed"], prm["max_mismatches"])[1]
        starts = (f[0] if f else 0, v[-1] if v else 0)
        prm["max_product"] = int(rs.choice([1, 30, 100, 4000, 2**31 - 1]))
        products = ribbit_amd.host_record_primer_products(seq, pair_row(oligos[0], oligos[1], *starts), ribbit_amd.product_params(**prm))
        assert pq.as_tuples(products) == [pq.pair_products(seq, oligos[0], oligos[1], *starts, prm)], (seed, case, prm, oligos[:2])
    assert found >= 10      # (by the contract: the cases are not all empty)


def test_defaults_and_struct_sizes():
    p = ribbit_amd.product_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == pq.DEFAULTS
    assert C.sizeof(ribbit_amd.ProductParams) == 16 == ribbit_amd.OLIGO_SITES_DT.itemsize and ribbit_amd.PRIMER_PRODUCTS_DT.itemsize == 32
    assert ribbit_amd.product_params(seed=6, max_sites=1).seed == 6
    with pytest.raises(TypeError, match="RibbitProductParams has no field 'flank'"):
        ribbit_amd.product_params(flank=3)
    with pytest.raises(ValueError, match="max_product 2147483648 does not fit int32"):
        ribbit_amd.product_params(max_product=2**31)
    for name in ("PRIMER_PRODUCTS_DT", "OLIGO_SITES_DT", "ProductParams", "product_params", "host_record_oligo_sites", "host_record_primer_products",
                 "bed_primer_products_text"):
        assert name in ribbit_amd.__all__


def test_every_refusal_and_the_limits_themselves():
    seq = (pq._L + pq._MID + pq._R).encode()
    row = pair_row(pq._L, pq._RB, 0, 38)
    for field, bad, message, good in (("seed", 5, "seed 5 is outside 6 .. 16", 6), ("seed", 17, "seed 17 is outside 6 .. 16", 16),
                                      ("max_mismatches", -1, "max_mismatches -1 is outside 0 .. 32", 0), ("max_mismatches", 33, "max_mismatches 33 is outside 0 .. 32", 32),
                                      ("max_product", 0, "max_product 0 is below 1", 1), ("max_product", -5, "max_product -5 is below 1", 2**31 - 1),
                                      ("max_sites", 0, "max_sites 0 is outside 1 .. 1024", 1), ("max_sites", 1025, "max_sites 1025 is outside 1 .. 1024", 1024)):
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"ribbit_host_record_primer_products error -1: {message}"):
            ribbit_amd.host_record_primer_products(seq, row, ribbit_amd.product_params(**{field: bad}))
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"ribbit_host_record_oligo_sites error -1: {message}"):
            ribbit_amd.host_record_oligo_sites(seq, [pq._L], ribbit_amd.product_params(**{field: bad}))
        prm = pq.params(**{field: good})
        assert pq.as_tuples(ribbit_amd.host_record_primer_products(seq, row, ribbit_amd.product_params(**prm))) == [pq.pair_products(seq, pq._L, pq._RB, 0, 38, prm)]
        assert pq.sites_as_lists(*ribbit_amd.host_record_oligo_sites(seq, [pq._L], ribbit_amd.product_params(**prm))) == pq.contract_sites(seq, [pq._L], prm)
    # an oligo shorter than the seed or longer than 32, by its index; exactly the seed and exactly 32 are taken
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: oligo 1: 14 bases, not seed 15 .. 32"):
        ribbit_amd.host_record_oligo_sites(seq, [pq._L, pq._L[:14]])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: oligo 0: 33 bases, not seed 15 .. 32"):
        ribbit_amd.host_record_oligo_sites(seq, ["A" * 33])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: oligo 2: 0 bases, not seed 6 .. 32"):
        ribbit_amd.host_record_oligo_sites(seq, [pq._L, pq._L, ""], ribbit_amd.product_params(seed=6))
    with pytest.raises(ValueError, match="oligo 1: .* has letters other than ACGT"):
        ribbit_amd.host_record_oligo_sites(seq, [pq._L, "ACGTNACGTACGTACGT"])
    long = (pq._L + pq._MID)[:32]
    assert pq.sites_as_lists(*ribbit_amd.host_record_oligo_sites(seq, [pq._L[3:], long])) == [(1, 0, [3], []), (1, 0, [0], [])]
    short = row.copy()
    short["right_length"] = 14
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: pair 1: a primer of 14 bases, not seed 15 .. 32"):
        ribbit_amd.host_record_primer_products(seq, np.concatenate([row, short]))
    # a target without a pair is not read beyond its left start
    none = short.copy()
    none["left_start"] = -1
    assert pq.as_tuples(ribbit_amd.host_record_primer_products(seq, np.concatenate([none, row]))) == [pq.NO_PRODUCTS, (1, 0, 0, 1, 1, 1, 0, 0)]
    assert len(ribbit_amd.host_record_primer_products(seq, row[:0])) == 0 and len(ribbit_amd.host_record_oligo_sites(seq, [])[0]) == 0
    assert pq.as_tuples(ribbit_amd.host_record_primer_products(b"", row)) == [pq.NO_PRODUCTS]
    with pytest.raises(TypeError, match="params: a ProductParams"):
        ribbit_amd.host_record_primer_products(seq, row, pq.DEFAULTS)
    L = ribbit_amd.load_library()
    out, p = C.c_void_p(), ribbit_amd.product_params()
    assert L.ribbit_host_record_primer_products(seq, len(seq), None, 1, C.byref(p), C.byref(out)) == -1 and b"null argument" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_primer_products(seq, len(seq), row.ctypes.data, 1, None, C.byref(out)) == -1
    assert L.ribbit_host_record_primer_products(seq, len(seq), row.ctypes.data, 1, C.byref(p), None) == -1
    assert L.ribbit_host_record_primer_products(None, 5, row.ctypes.data, 1, C.byref(p), C.byref(out)) == -1 and b"bad sequence" in L.ribbit_hip_last_error()
    assert L.ribbit_host_record_primer_products(seq, -1, row.ctypes.data, 1, C.byref(p), C.byref(out)) == -1 and b"a record of -1 bases" in L.ribbit_hip_last_error()


BED = "".join(f"rec one\t{s}\t{e}\tAC\t2\t{e - s}\t{(e - s) // 2}\t1.00\t+\tP\t{e - s}=\n" for s, e in ((260, 280), (0, 40), (1100, 1130)))


def test_the_text_byte_for_byte():
    seq = pc.clean_record(900, 3)
    seq = seq[:480] + seq[60:480] + seq[480:]      # the first row with its flanks a second time: its pair has other products
    rows = ribbit_amd.bed_intervals(BED).tolist()
    pairs = ribbit_amd.host_record_primer_pairs(seq, rows, rows)
    assert [int(s) >= 0 for s in pairs["left_start"]] == [True, False, True]
    products = ribbit_amd.host_record_primer_products(seq, pairs)
    want = pq.record_primer_products(seq, pp.as_tuples(pairs))
    assert pq.as_tuples(products) == want and want[0][4] - want[0][5] >= 1 and want[1] == pq.NO_PRODUCTS and want[2][4:7] == (1, 1, 0)
    text = ribbit_amd.bed_primer_products_text(BED, pairs, products).decode()
    assert text == pq.product_lines(BED, pp.as_tuples(pairs), want)
    assert ribbit_amd.bed_primer_products_text(BED[:-1], pairs, products).decode() == text          # a last line without its newline counts
    lines = [line.split("\t") for line in text.splitlines()]
    assert all(len(line) == 38 for line in lines)
    # the first 32 columns are the pairs' text, from the same code
    assert ["\t".join(line[:32]) for line in lines] == ribbit_amd.bed_primer_pairs_text(BED, pairs).decode().splitlines()
    assert lines[1][32:] == ["."] * 6 and lines[2][32:] == ["1", "0", "0", "1", "0", "0"] and int(lines[0][36]) >= 1 and int(lines[0][37]) > 0
    # products == -1: the counts stay, the last two are dots
    few = ribbit_amd.host_record_primer_products(seq, pairs, ribbit_amd.product_params(max_sites=1))
    assert few["products"][0] == -1 and few["products"][2] == 1
    line = ribbit_amd.bed_primer_products_text(BED, pairs, few).decode().splitlines()[0].split("\t")
    assert line[32:36] == lines[0][32:36] and line[36:] == [".", "."]
    assert ribbit_amd.bed_primer_products_text("", pairs[:0], products[:0]) == b""
    big = np.zeros(1, ribbit_amd.PRIMER_PRODUCTS_DT)
    for name, value in zip(pq.FIELDS, (2**31 - 1,) * 5 + (1, 2**31 - 1, 0)):
        big[name] = value
    assert ribbit_amd.bed_primer_products_text("x", pairs[:1], big).endswith(b"\t2147483647" * 4 + b"\t2147483646\t2147483647\n")
    # the refusals
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 3 lines, not the 2 of the rows"):
        ribbit_amd.bed_primer_products_text(BED, pairs[:2], products[:2])
    with pytest.raises(ValueError, match="3 pairs and 2 products"):
        ribbit_amd.bed_primer_products_text(BED, pairs, products[:2])
    bad = pairs.copy()
    bad["right_length"][0] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: row 0: a primer of 33 bases, not 1 .. 32"):
        ribbit_amd.bed_primer_products_text(BED, bad, products)
    L = ribbit_amd.load_library()
    out, n = C.c_void_p(), C.c_size_t()
    f = L.ribbit_bed_primer_products_text
    assert f(b"x", 1, None, products.ctypes.data, 1, C.byref(out), C.byref(n)) == -1 and f(b"x", 1, pairs.ctypes.data, None, 1, C.byref(out), C.byref(n)) == -1
    assert f(b"x", 1, pairs.ctypes.data, products.ctypes.data, 1, None, C.byref(n)) == -1 and b"null argument" in L.ribbit_hip_last_error()


def test_with_random_background():
    seq, truth = simulate_sequence(30000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    again, _ = simulate_sequence(30000, 7, 2, 30, n_block_rate=0.3, lower_rate=0.2)
    out = with_random_background(seq, truth, 5)
    assert seq == again and len(out) == len(seq) and out == with_random_background(seq, truth, 5) != with_random_background(seq, truth, 6)
    a, b = np.frombuffer(seq, np.uint8), np.frombuffer(out, np.uint8)
    inside = np.zeros(len(a), bool)
    for start, end, *_ in truth:
        inside[start:end] = True
    assert inside.any() and np.array_equal(a[inside], b[inside])
    is_n = a == ord("N")
    assert is_n.any() and np.array_equal(is_n, b == ord("N")) and any(seq[s:e].islower() for s, e, *_ in truth)
    outside = ~inside & ~is_n
    assert set(b[outside].tolist()) == set(b"ACGT") and 0.7 < (a[outside] != b[outside]).mean() < 0.8
    # the tiled unit is gone: a flank's 15 bases recur at every locus before, and nowhere after
    unit = seq[truth[3][0] - 15:truth[3][0]]
    assert seq.count(unit) > 10 and out.count(out[truth[3][0] - 15:truth[3][0]]) == 1


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
    _dies(["--primer-product-flank", "5"], "--primer-product-flank needs --primer-product-bed")
    _dies(["-i", "in.fa", "--primer-product-flank=5"], "--primer-product-flank needs --primer-product-bed")
    _dies(["--primer-product-flank", "5", "--primer-pair-bed", "b"], "--primer-product-flank needs --primer-product-bed")
    _dies(["--primer-pair-flank", "5", "--primer-product-bed", "b"], "--primer-pair-flank needs --primer-pair-bed")
    # the first in the order of the outputs
    _dies(["--primer-product-flank", "5", "--primer-pair-flank", "5"], "--primer-pair-flank needs --primer-pair-bed")
    _fails(["--primer-product-bed", tmp_path / "missing" / "out", "--primer-product-flank", "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values_and_file_names(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("1001", "-1", "x", "10000", "1e3", "", "+5"):
        _dies(["-i", "in.fa", "--primer-product-bed", "b", "--primer-product-flank", value],
              f"--primer-product-flank wants a whole number of bases (0 .. 1000), got '{value}'")
    for value in ("0", "1000", "0200"):
        _dies(["-i", tmp_path / "in.fa", "--primer-product-bed", out, "--primer-product-flank", value], f"--primer-product-bed: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--primer-product-bed", "b", "--primer-product-flank"], "the required argument for option '--primer-product-flank' is missing")
    _dies(["--primer-product-bed="], "--primer-product-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-product-bed", ""], "--primer-product-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-product-bed"], "the required argument for option '--primer-product-bed' is missing")
    # the contract's parameters are the ABI's and Python's, not the tool's
    for option in ("--primer-product-seed", "--primer-product-max-sites", "--primer-products-bed"):
        _dies(["-i", "in.fa", "--primer-product-bed", "x", option, "3"], f"unrecognised option '{option}'")


@needs_tool
def test_cli_the_file_is_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    options = EARLIER_OUTPUTS + ["--primer-product-bed"]
    assert len(options) == 19
    for bad in (17, 18):
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
    names = ["--primer-pair-bed", "--primer-pair-flank", "--primer-product-bed", "--primer-product-flank"]
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[1]:at[2]].endswith("Default: 200") and r.stderr[at[3]:].rstrip("\n").endswith("Default: 200")
    entry = " ".join(r.stderr[at[2]:at[3]].split())
    assert "27 columns" in entry and "Only the record itself is searched, not the other records of the input" in entry and "Scanner.record_oligo_sites" in entry
