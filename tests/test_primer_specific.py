"""The specific primer pairs without a GPU: the five constructed records whose values include/ribbit_hip.h pins, through both forms
of the plain statement (tests/primer_specific_contract.py) and through the host twin, field by field; the twin against that
statement on random records; the text byte for byte; every refusal; and ribbit-hip's handling of --primer-specific-bed and
--primer-specific-flank up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

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
                   "--composition-track", "--primer-bed", "--primer-pair-bed", "--primer-product-bed"]
# mostly bases, so that windows hold candidates, with N, IUPAC letters and other bytes among them
MOSTLY_BASES = b"ACGTacgt" * 40 + b"NnRYx-"


def _twin(seq, rows, targets, prm=None, pair=None, product=None):
    got = ribbit_amd.host_record_specific_primer_pairs(seq, rows, targets, ribbit_amd.primer_params(**(prm or {})), ribbit_amd.primer_pair_params(**(pair or {})),
                                                       ribbit_amd.product_params(**(product or {})))
    for arr, dt in zip(got, (ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PRIMER_PRODUCTS_DT, ribbit_amd.PRIMER_SPECIFIC_DT)):
        assert arr.dtype == dt and arr.shape == (len(targets),)
    return tuple(ps.as_tuples(a) for a in got)


def _contract(seq, rows, targets, prm=None, pair=None, product=None, loops=False):
    return ps.record_specific_primer_pairs(seq, rows, targets, pc.params(**(prm or {})), pp.pair_params(**(pair or {})), pq.params(**(product or {})), loops=loops)


def _same(got, want, what):
    for g, w, fields in zip(got, want, (pp.FIELDS, pq.FIELDS, ps.FIELDS)):
        assert len(g) == len(w), what
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (what, i, [(f, x, y) for f, x, y in zip(fields, a, b) if x != y])


def test_the_five_pinned_cases():
    cases = ps.constructed()
    assert list(cases) == list(ps.PINNED) and len(cases) == 5
    seen = set()
    for name, (record, fields) in cases.items():
        want = _contract(record, [], [ps.TARGET], product=fields, loops=True)
        assert want == _contract(record, [], [ps.TARGET], product=fields, loops=False), name
        (p,), (q,), (s,) = want
        assert (s[:6], (p[0], p[1], p[6], p[7])) == ps.PINNED[name], name
        assert s[1] == s[2] + s[3] + s[4] == p[30] and s[6:] == (0, 0)
        for seq in (record, record.lower()):
            _same(_twin(seq, [], [ps.TARGET], product=fields), want, name)
        seen |= {"first" if s[0] == 0 else "later" if s[0] > 0 else "none with other" if s[4] > 0 else "none", "over" if s[3] > 0 else ""}
        if s[0] >= 0:      # the chosen pair is specific, and it is the pair of that place in the order of the choice
            assert q[4] - q[5] == 0 and q[4] >= 0 and s[2] >= 1
        else:
            assert p[:25] == pc.NO_PRIMER * 2 + (0,) * 13 and q == pq.NO_PRODUCTS and s[2] == 0
    assert {"first", "later", "none with other", "over"} <= seen
    # place 0 is record_primer_pairs' own pair, whatever becomes of it
    record, _ = cases["best pair copied"]
    best = pp.record_primer_pairs(record, [], [ps.TARGET])[0]
    (p,), _, (s,) = _contract(record, [], [ps.TARGET])
    assert s[0] == 2 and p[:12] != best[:12] and p[25:] == best[25:]
    assert s[5] == pq.record_primer_products(record, [best])[0][4] - 1


@pytest.mark.parametrize("seed", range(4))
def test_random_records_with_edge_targets(seed):
    """records of 300 .. 3,000 bases with N, lower case and IUPAC letters, targets at the record's ends and at word edges, reversed,
    empty and out of range; a part of each record a second time, so that pairs are passed over; every parameter set drawn"""
    rs = np.random.RandomState(40 + seed)
    chosen = later = none_of_some = 0
    for case in range(6):
        length = int(rs.randint(300, 3001))
        seq = pc.random_record(length, 7 * seed + case, MOSTLY_BASES if case else pc.ALPHABET)
        if case % 2 == 0:
            seq = (seq[:length // 2] + seq[:length // 2])[:length]
        rows = pc.random_targets(length, rs, 4, longest=40).tolist()
        targets = pc.edge_targets(length) + pc.random_targets(length, rs, 6, longest=60).tolist()
        prm = dict(flank=int(rs.choice([0, 30, 200, 1000])), gc_clamp=int(rs.randint(2)), tm_min=520, tm_max=660) if rs.randint(2) else {}
        pair = dict(shortlist=int(rs.randint(1, 9))) if rs.randint(2) else dict(pp.LOOSE, shortlist=int(rs.randint(1, 9)))
        product = dict(seed=int(rs.randint(6, 16)), max_mismatches=int(rs.choice([0, 2, 32])), max_product=int(rs.choice([300, 4000, 2**31 - 1])),
                       max_sites=int(rs.choice([1, 2, 64])))
        want = _contract(seq, rows, targets, prm, pair, product)
        _same(_twin(seq, rows, targets, prm, pair, product), want, (seed, case, prm, pair, product))
        chosen += sum(s[0] >= 0 for s in want[2])
        later += sum(s[0] > 0 for s in want[2])
        none_of_some += sum(s[0] < 0 < s[1] for s in want[2])
    assert chosen > 0 and later + none_of_some > 0, (chosen, later, none_of_some)      # (by the contract: pairs are chosen, and pairs are passed over)


def test_the_two_forms_of_the_statement_agree():
    seq = pc.random_record(1500, 3, MOSTLY_BASES)
    seq = seq[:700] + seq[:700] + seq[1400:]
    targets = pc.random_targets(len(seq), np.random.RandomState(1), 8, longest=50).tolist()
    a = _contract(seq, [(200, 230)], targets, loops=True)
    assert a == _contract(seq, [(200, 230)], targets, loops=False) and any(s[1] > 0 for s in a[2])


BED = "".join(f"rec one\t{s}\t{e}\tAC\t2\t{e - s}\t{(e - s) // 2}\t1.00\t+\tP\t{e - s}=\n" for s, e in ((1500, 1540), (0, 40), (700, 730)))


def test_the_text_byte_for_byte():
    record, _ = ps.constructed()["best pair copied"]
    rows = ribbit_amd.bed_intervals(BED).tolist()
    pairs, products, specific = ribbit_amd.host_record_specific_primer_pairs(record, rows, rows)
    want = _contract(record, rows, rows)
    assert (ps.as_tuples(pairs), ps.as_tuples(products), ps.as_tuples(specific)) == want
    assert [s[0] for s in want[2]] == [2, -1, 0]
    text = ribbit_amd.bed_primer_specific_text(BED, pairs, products, specific).decode()
    assert text == ps.specific_lines(BED, *want)
    assert ribbit_amd.bed_primer_specific_text(BED[:-1], pairs, products, specific).decode() == text      # a last line without its newline counts
    lines = [line.split("\t") for line in text.splitlines()]
    assert all(len(line) == 42 for line in lines)
    # the first 38 columns are the products' text of the chosen pairs, from the same code
    assert ["\t".join(line[:38]) for line in lines] == ribbit_amd.bed_primer_products_text(BED, pairs, products).decode().splitlines()
    assert lines[0][38:] == ["2", "26", "0", "18"] and lines[1][11:29] == ["."] * 18 and lines[1][32:39] == ["."] * 7 and lines[1][39:] == ["0", "0", "0"]
    assert lines[2][38] == "0" and lines[2][36] == "0"
    # no pair though pairs are admissible: the counts stay
    both, _ = ps.constructed()["both flanks copied"]
    none = ribbit_amd.host_record_specific_primer_pairs(both, [], [ps.TARGET])
    line = ribbit_amd.bed_primer_specific_text("x", *none).decode()
    by_contract = _contract(both, [], [ps.TARGET])
    passed = by_contract[0][0][27:29]
    assert min(passed) >= 8 and line == "x" + "\t." * 18 + f"\t{passed[0]}\t{passed[1]}\t44" + "\t." * 7 + "\t0\t0\t44\n" == ps.specific_lines("x", *by_contract)
    assert ribbit_amd.bed_primer_specific_text("", pairs[:0], products[:0], specific[:0]) == b""
    # the refusals
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 3 lines, not the 2 of the rows"):
        ribbit_amd.bed_primer_specific_text(BED, pairs[:2], products[:2], specific[:2])
    with pytest.raises(ValueError, match="3 pairs, 2 products and 3 summaries"):
        ribbit_amd.bed_primer_specific_text(BED, pairs, products[:2], specific)
    bad = pairs.copy()
    bad["right_length"][0] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: row 0: a primer of 33 bases, not 1 .. 32"):
        ribbit_amd.bed_primer_specific_text(BED, bad, products, specific)
    L = ribbit_amd.load_library()
    out, n = C.c_void_p(), C.c_size_t()
    f = L.ribbit_bed_primer_specific_text
    args = [pairs.ctypes.data, products.ctypes.data, specific.ctypes.data]
    for k in range(3):
        assert f(b"x", 1, *(None if j == k else a for j, a in enumerate(args)), 1, C.byref(out), C.byref(n)) == -1 and b"null argument" in L.ribbit_hip_last_error()
    assert f(b"x", 1, *args, 1, None, C.byref(n)) == -1


def test_every_refusal_and_the_empty_cases():
    record, _ = ps.constructed()["undisturbed"]
    call = lambda **k: ribbit_amd.host_record_specific_primer_pairs(record, [], [ps.TARGET], k.get("prm"), k.get("pair"), k.get("product"))
    label = "ribbit_host_record_specific_primer_pairs error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "flank 1001 is outside 0 .. 1000"):
        call(prm=ribbit_amd.primer_params(flank=1001))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "shortlist 9 is outside 1 .. 8"):
        call(pair=ribbit_amd.primer_pair_params(shortlist=9))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "max_pair_end 33 is outside 0 .. 32"):
        call(pair=ribbit_amd.primer_pair_params(max_pair_end=33))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "max_sites 1025 is outside 1 .. 1024"):
        call(product=ribbit_amd.product_params(max_sites=1025))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "seed 5 is outside 6 .. 16"):
        call(product=ribbit_amd.product_params(seed=5))
    # a shortlisted primer may not be shorter than the seed; exactly the seed is taken
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "min_length 14 is below seed 15"):
        call(prm=ribbit_amd.primer_params(min_length=14))
    pairs, _, specific = call(prm=ribbit_amd.primer_params(min_length=15))
    assert specific["place"][0] == 0 and pairs["left_start"][0] >= 0
    for wrong, message in ((dict(prm=pc.DEFAULTS), "params: a PrimerParams"), (dict(pair=pp.PAIR_DEFAULTS), "pair_params: a PrimerPairParams"),
                           (dict(product=pq.DEFAULTS), "product_params: a ProductParams")):
        with pytest.raises(TypeError, match=message):
            call(**wrong)
    # no targets, an empty record, targets without candidates
    assert all(len(a) == 0 for a in ribbit_amd.host_record_specific_primer_pairs(record, [], []))
    empty = (pc.NO_PRIMER * 2 + (0,) * 20, pq.NO_PRODUCTS, (-1, 0, 0, 0, 0, 0, 0, 0))
    got = _twin(b"", [], [(0, 5), (-3, 2)])
    assert got == tuple([e, e] for e in empty)
    assert _twin(b"N" * 500, [], [(200, 220)]) == tuple([e] for e in empty)
    L = ribbit_amd.load_library()
    f = L.ribbit_host_record_specific_primer_pairs
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    p, q, r = ribbit_amd.primer_params(), ribbit_amd.primer_pair_params(), ribbit_amd.product_params()
    tg = np.array([ps.TARGET], np.int32)
    good = [record, len(record), None, 0, tg.ctypes.data, 1, C.byref(p), C.byref(q), C.byref(r), C.byref(a), C.byref(b), C.byref(c)]
    for k in (4, 6, 7, 8, 9, 10, 11):
        assert f(*(None if j == k else v for j, v in enumerate(good))) == -1 and b"null argument" in L.ribbit_hip_last_error(), k
    assert f(None, 5, *good[2:]) == -1 and b"bad sequence" in L.ribbit_hip_last_error()
    assert f(record, -1, *good[2:]) == -1 and b"a record of -1 bases" in L.ribbit_hip_last_error()
    assert L.ribbit_hip_record_specific_primer_pairs(None, *good[2:]) == -1 and b"null handle" in L.ribbit_hip_last_error()
    assert L.ribbit_hip_debug_set_specific_batch(None, 2) == -1


def test_names_sizes_and_the_binding():
    for name in ("PRIMER_SPECIFIC_DT", "host_record_specific_primer_pairs", "bed_primer_specific_text"):
        assert name in ribbit_amd.__all__ and hasattr(ribbit_amd, name)
    assert ribbit_amd.PRIMER_SPECIFIC_DT.itemsize == 32 and ribbit_amd.PRIMER_SPECIFIC_DT.names == ps.FIELDS
    assert hasattr(ribbit_amd.Scanner, "record_specific_primer_pairs") and hasattr(ribbit_amd.Scanner, "debug_set_specific_batch")
    for symbol in ("ribbit_hip_record_specific_primer_pairs", "ribbit_host_record_specific_primer_pairs", "ribbit_primer_specific_free",
                   "ribbit_hip_debug_set_specific_batch", "ribbit_bed_primer_specific_text"):
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
    _dies(["--primer-specific-flank", "5"], "--primer-specific-flank needs --primer-specific-bed")
    _dies(["-i", "in.fa", "--primer-specific-flank=5"], "--primer-specific-flank needs --primer-specific-bed")
    _dies(["--primer-specific-flank", "5", "--primer-product-bed", "b"], "--primer-specific-flank needs --primer-specific-bed")
    _dies(["--primer-product-flank", "5", "--primer-specific-bed", "b"], "--primer-product-flank needs --primer-product-bed")
    # the first in the order of the outputs
    _dies(["--primer-specific-flank", "5", "--primer-product-flank", "5"], "--primer-product-flank needs --primer-product-bed")
    _fails(["--primer-specific-bed", tmp_path / "missing" / "out", "--primer-specific-flank", "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values_and_file_names(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("1001", "-1", "x", "10000", "1e3", "", "+5"):
        _dies(["-i", "in.fa", "--primer-specific-bed", "b", "--primer-specific-flank", value],
              f"--primer-specific-flank wants a whole number of bases (0 .. 1000), got '{value}'")
    for value in ("0", "1000", "0200"):
        _dies(["-i", tmp_path / "in.fa", "--primer-specific-bed", out, "--primer-specific-flank", value], f"--primer-specific-bed: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--primer-specific-bed", "b", "--primer-specific-flank"], "the required argument for option '--primer-specific-flank' is missing")
    _dies(["--primer-specific-bed="], "--primer-specific-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-specific-bed", ""], "--primer-specific-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-specific-bed"], "the required argument for option '--primer-specific-bed' is missing")
    # the contract's parameters are the ABI's and Python's, not the tool's
    for option in ("--primer-specific-seed", "--primer-specific-max-sites", "--primer-specifics-bed"):
        _dies(["-i", "in.fa", "--primer-specific-bed", "x", option, "3"], f"unrecognised option '{option}'")


@needs_tool
def test_cli_the_file_is_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    options = EARLIER_OUTPUTS + ["--primer-specific-bed"]
    assert len(options) == 20
    for bad in (18, 19):
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
    names = ["--primer-product-bed", "--primer-product-flank", "--primer-specific-bed", "--primer-specific-flank"]
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[1]:at[2]].endswith("Default: 200") and r.stderr[at[3]:].rstrip("\n").endswith("Default: 200")
    entry = " ".join(r.stderr[at[2]:at[3]].split())
    assert "31 columns" in entry and "Only the record itself is searched, not the other records of the input" in entry and "there is no fallback" in entry
