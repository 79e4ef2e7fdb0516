"""Primer pairs chosen together without a GPU: the pinned values of the duplex and the hairpin through ribbit_host_oligo_duplex /
ribbit_host_oligo_hairpin and through the plain statement (tests/primer_pairs_contract.py); ribbit_host_record_primer_pairs against
that statement, exactly; what each limit does; the text byte for byte; every refusal with its text; and ribbit-hip's handling of
--primer-pair-bed and --primer-pair-flank up to the point where it would touch a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import primer_pairs_contract as pp
import primers_contract as pc
import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
EARLIER_OUTPUTS = ["--masked-fasta", "--repeat-fasta", "--loci-bed", "--density-bedgraph", "--overlap-bed", "--overlap-summary", "--best-bed", "--class-bed",
                   "--motif-summary", "--compound-bed", "--interruption-bed", "--purity-bed", "--nearest-bed", "--nearest-other-bed", "--composition-bed",
                   "--composition-track", "--primer-bed"]
# small oligos make every rule bite on short records (test_primers.py); their limits are scaled down with them
SMALL = dict(flank=30, min_length=5, max_length=8, opt_length=6, tm_min=0, tm_opt=150, tm_max=400, gc_min_percent=20, gc_max_percent=80)
SMALL_PAIR = dict(max_self_any=3, max_self_end=2, max_hairpin=2, max_pair_any=3, max_pair_end=2, max_tm_difference=60)
NO_PAIR = pc.NO_PRIMER * 2 + (0,) * 13
LIMITS = ("max_self_any", "max_self_end", "max_hairpin", "max_pair_any", "max_pair_end")


def twin(seq, rows, targets, fields=None, pair=None):
    got = ribbit_amd.host_record_primer_pairs(seq, rows, targets, ribbit_amd.primer_params(**(fields or {})), ribbit_amd.primer_pair_params(**(pair or {})))
    assert got.dtype == ribbit_amd.PRIMER_PAIRS_DT and got.shape == (len(targets),) and got.dtype.names == pp.FIELDS
    return pp.as_tuples(got)


def check(seq, rows, targets, what=None, loops=False, fields=None, pair=None):
    """the twin equals the contract, in its array form and, where asked, in its loops over letters"""
    got = twin(seq, rows, targets, fields, pair)
    prm, prs = pc.params(**(fields or {})), pp.pair_params(**(pair or {}))
    want = pp.record_primer_pairs_without_loops(seq, rows, targets, prm, prs)
    assert got == want, (len(seq), what, fields, pair)
    if loops:
        assert pp.record_primer_pairs(seq, rows, targets, prm, prs) == want, (len(seq), what, fields, pair)
    for r in want:      # what holds for every record
        assert (r[0] >= 0) == (r[6] >= 0) == (r[30] >= 1) and r[31] == 0 and r[27] <= r[25] and r[28] <= r[26]
        assert r[29] == min(prs["shortlist"], r[27]) * min(prs["shortlist"], r[28]) and r[30] <= r[29]
        if r[0] < 0:
            assert r[:25] == NO_PAIR
        else:
            assert r[12] == r[3] + r[9] + r[13] and r[13] == abs(r[2] - r[8]) <= prs["max_tm_difference"] and r[14] == r[6] + r[7] - r[0]
            assert r[15] < min(prs["shortlist"], r[27]) and r[16] < min(prs["shortlist"], r[28])
            assert all(v <= prs[n] for v, n in zip(r[17:20] + r[20:23] + r[23:25], ("max_self_any", "max_self_end", "max_hairpin") * 2 + ("max_pair_any", "max_pair_end")))
    return want


def test_the_pinned_values():
    for (a, b), want in pp.DUPLEX_VECTORS.items():
        assert ribbit_amd.oligo_duplex(a, b) == want == pp.duplex(a, b) == pp.duplex_packed(a, b), (a, b)
        assert ribbit_amd.oligo_duplex(a.lower(), b.encode()) == want
    for a, want in pp.HAIRPIN_VECTORS.items():
        assert ribbit_amd.oligo_hairpin(a) == want == pp.hairpin(a) == ribbit_amd.oligo_hairpin(a.lower().encode()), a


def test_any_and_end_are_symmetric():
    rs = np.random.RandomState(5)
    for _ in range(300):
        a, b = ("".join("ACGT"[c] for c in rs.randint(0, 4, rs.randint(1, 33))) for _ in range(2))
        d = ribbit_amd.oligo_duplex(a, b)
        assert d == ribbit_amd.oligo_duplex(b, a) == pp.duplex(a, b) == pp.duplex_packed(a, b) and 0 <= d[1] <= d[0] <= min(len(a), len(b)), (a, b)
        assert ribbit_amd.oligo_hairpin(a) == pp.hairpin(a) <= max(0, (len(a) - pp.HAIRPIN_LOOP) // 2)
    # a duplex of an oligo with its reverse complement is complete
    assert ribbit_amd.oligo_duplex(a, pp.reverse_complement(a)) == (len(a), len(a))


def test_the_defaults_and_the_layout():
    p = ribbit_amd.primer_pair_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == pp.PAIR_DEFAULTS
    assert C.sizeof(p) == 28 and ribbit_amd.PRIMER_PAIRS_DT.itemsize == 128 and len(pp.FIELDS) == 32 and ribbit_amd.PRIMER_PAIRS_DT.names == pp.FIELDS
    assert ribbit_amd.primer_pair_params(shortlist=3, max_hairpin=0).shortlist == 3
    with pytest.raises(TypeError):
        ribbit_amd.primer_pair_params(max_hairpins=7)
    for name in ("PRIMER_PAIRS_DT", "PrimerPairParams", "primer_pair_params", "host_record_primer_pairs", "bed_primer_pairs_text", "oligo_duplex", "oligo_hairpin"):
        assert name in ribbit_amd.__all__
    assert hasattr(ribbit_amd.Scanner, "record_primer_pairs")


def test_every_refusal():
    L = ribbit_amd.load_library()
    call = lambda pair, fields=None: ribbit_amd.host_record_primer_pairs(b"ACGT", [], [(0, 1)], ribbit_amd.primer_params(**(fields or {})), ribbit_amd.primer_pair_params(**pair))
    bad = [(dict(shortlist=0), "shortlist 0 is outside 1 .. 8"), (dict(shortlist=9), "shortlist 9 is outside 1 .. 8"),
           (dict(max_tm_difference=-1), "max_tm_difference -1 is outside 0 .. 2000"), (dict(max_tm_difference=2001), "max_tm_difference 2001 is outside 0 .. 2000")]
    bad += [(dict({n: v}), f"{n} {v} is outside 0 .. 32") for n in LIMITS for v in (-1, 33)]
    for pair, message in bad:
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: {message}$"):
            call(pair)
    # the primer parameters are checked as record_primers checks them, and first
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: flank 1001 is outside 0 .. 1000$"):
        call(dict(shortlist=0), dict(flank=1001))
    # the limits themselves are accepted
    for pair in [dict(shortlist=1), dict(shortlist=8), dict(max_tm_difference=0), dict(max_tm_difference=2000)] + [dict({n: v}) for n in LIMITS for v in (0, 32)]:
        assert len(call(pair)) == 1
    out, prm, prs = C.c_void_p(), ribbit_amd.primer_params(), ribbit_amd.primer_pair_params()
    iv = np.zeros(2, np.int32)
    f = L.ribbit_host_record_primer_pairs
    assert f(b"ACGT", 4, None, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(prs), C.byref(out)) == -1
    assert f(b"ACGT", 4, iv.ctypes.data, 1, None, 1, C.byref(prm), C.byref(prs), C.byref(out)) == -1
    assert f(b"ACGT", 4, iv.ctypes.data, 1, iv.ctypes.data, 1, None, C.byref(prs), C.byref(out)) == -1
    assert f(b"ACGT", 4, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), None, C.byref(out)) == -1
    assert f(b"ACGT", 4, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(prs), None) == -1
    assert b"null argument" in L.ribbit_hip_last_error()
    assert f(None, 4, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(prs), C.byref(out)) == -1
    assert b"bad sequence" in L.ribbit_hip_last_error()
    assert f(b"ACGT", 2**31, iv.ctypes.data, 1, iv.ctypes.data, 1, C.byref(prm), C.byref(prs), C.byref(out)) == -1
    assert b"a record of 2147483648 bases" in L.ribbit_hip_last_error()
    with pytest.raises(TypeError):
        ribbit_amd.host_record_primer_pairs(b"ACGT", [], [(0, 1)], None, pp.PAIR_DEFAULTS)
    # no targets, no rows, no bases: no errors
    assert len(ribbit_amd.host_record_primer_pairs(b"ACGT", [(0, 2)], [])) == 0
    assert twin(b"", [(0, 5)], [(0, 5), (-2, 2)]) == [NO_PAIR + (0,) * 7] * 2
    assert f(None, 0, None, 0, None, 0, C.byref(prm), C.byref(prs), C.byref(out)) == 0
    L.ribbit_primer_pairs_free(out)
    L.ribbit_primer_pair_params_default(None)
    # the oligos
    a, e = C.c_int32(), C.c_int32()
    for x, y in ((b"", b"ACGT"), (b"ACGT", b""), (b"ACGN", b"ACGT"), (b"ACGT", b"AC GT"), (b"A" * 33, b"ACGT"), (None, b"ACGT"), (b"ACGT", None)):
        assert L.ribbit_host_oligo_duplex(x, y, C.byref(a), C.byref(e)) == -1
        assert b"an oligo is 1 .. 32 letters of ACGTacgt" in L.ribbit_hip_last_error()
    for x in (b"", b"ACGU", b"C" * 33, None):
        assert L.ribbit_host_oligo_hairpin(x, C.byref(a)) == -1
    assert L.ribbit_host_oligo_duplex(b"ACGT", b"ACGT", None, C.byref(e)) == -1 and L.ribbit_host_oligo_hairpin(b"ACGT", None) == -1
    assert ribbit_amd.oligo_duplex("A" * 32, "T" * 32) == (32, 32) and ribbit_amd.oligo_hairpin("A" * 14 + "CCCC" + "T" * 14) == 14
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: an oligo is 1 .. 32 letters of ACGTacgt"):
        ribbit_amd.oligo_hairpin("ACGTN")


@pytest.mark.parametrize("length", (0, 1, 17, 64, 65, 1000))
def test_host_twin_on_the_edge_targets(length):
    found = 0
    for name, seq in (("random", pc.random_record(length, length)), ("clean", pc.clean_record(length, length)), ("all N", b"N" * length)):
        rows = [(5, 9), (40, 70), (length - 20, length + 5)]
        for flank in (0, 17, 200, 1000):
            if length == 1000 and flank == 1000 and name != "clean":
                continue
            small = check(seq, rows, pc.edge_targets(length), (name, flank), loops=length <= 65 and name == "clean", fields=dict(SMALL, flank=flank), pair=SMALL_PAIR)
            found += sum(r[0] >= 0 for r in small)
            if name == "all N" or flank == 0:
                assert all(r == NO_PAIR + (0,) * 7 for r in small)
            if name == "clean":
                found += sum(r[0] >= 0 for r in check(seq, rows, pc.edge_targets(length), (name, flank), fields=dict(flank=flank)))
    # (a record of 17 bases has no room for two flanks of 5 beside the rows; in the longest some targets have a pair)
    assert found > 0 if length == 1000 else found == 0 if length <= 17 else True, found


@pytest.fixture(scope="module")
def records():
    rs = np.random.RandomState(23)
    clean, random = pc.clean_record(12000, 31), pc.random_record(12000, 32, b"ACGTacgtACGTacgtACGTacgtN")
    return {"clean": (clean, pc.random_targets(len(clean), rs, 12, longest=40), pc.random_targets(len(clean), rs, 200)),
            "random": (random, pc.random_targets(len(random), rs, 12, longest=40), pc.random_targets(len(random), rs, 200))}


@pytest.mark.parametrize("name", ("clean", "random"))
def test_the_defaults_on_random_records(records, name):
    seq, rows, targets = records[name]
    want = check(seq, rows, targets, name)
    paired = sum(r[0] >= 0 for r in want)
    assert paired >= (150 if name == "clean" else 10), paired
    assert pp.record_primer_pairs(seq, rows, targets[:4]) == want[:4]
    for (s, e), r in zip(targets.tolist(), want):
        s1, e1, lo, hi = pc.clip(s, e, 200, len(seq))
        assert r[0] == -1 or (lo <= r[0] and r[0] + r[1] <= s1 and e1 <= r[6] and r[6] + r[7] <= hi)


def test_loose_limits_are_the_two_primers_of_record_primers(records):
    """with limits that refuse nothing and a shortlist of one the pair is record_primers' two primers wherever both sides have
    one, and the counts are its counts whatever the limits"""
    for name, (seq, rows, targets) in records.items():
        loose = check(seq, rows, targets, name, pair=pp.LOOSE)
        alone = pc.as_tuples(ribbit_amd.host_record_primers(seq, rows, targets))
        assert sum(a[0] >= 0 and a[6] >= 0 for a in alone) >= 10
        for r, a in zip(loose, alone):
            assert r[25:29] == a[12:] * 2      # (everything admissible passes)
            assert pp.primers_of(r) == a if a[0] >= 0 and a[6] >= 0 else r[:25] == NO_PAIR
            assert (r[15], r[16], r[29]) == ((0, 0, 1) if r[0] >= 0 else (0, 0, 0))
        for r, a in zip(twin(seq, rows, targets), alone):
            assert r[25:27] == a[12:]


# a record of 900 clean bases per seed, three targets; found with the contract: with every other limit loose, this limit at its
# default moves the pair away from record_primers' two primers, which the same parameters with this limit loose too return
TARGETS = [(300, 320), (440, 470), (560, 600)]
BY_LIMIT = {"max_self_any": (1000, 0), "max_self_end": (1000, 2), "max_hairpin": (1000, 2), "max_pair_end": (1000, 1), "max_pair_any": (1001, 1)}


def _value_of(limit, a, b):
    """what the limit bounds, of the pair of oligos a (left) and b (right)"""
    if limit.startswith("max_pair"):
        return ribbit_amd.oligo_duplex(a, b)[limit.endswith("end")]
    return max(ribbit_amd.oligo_hairpin(o) if limit == "max_hairpin" else ribbit_amd.oligo_duplex(o, o)[limit.endswith("end")] for o in (a, b))


@pytest.mark.parametrize("limit", sorted(BY_LIMIT) + ["max_tm_difference"])
def test_each_limit_alone_moves_the_pair(limit):
    if limit == "max_tm_difference":      # (record_primers' two primers melt more than 3 degrees apart only with an optimum at an end of the range and few candidates)
        seq, targets, fields = pc.clean_record(700, 2045), [(220, 240)], dict(flank=26, tm_opt=570)
    else:
        seed, at = BY_LIMIT[limit]
        seq, targets, fields = pc.clean_record(900, seed), TARGETS[at:at + 1], {}
    base = dict(pp.LOOSE, shortlist=8)
    (alone,) = pc.as_tuples(ribbit_amd.host_record_primers(seq, TARGETS, targets, ribbit_amd.primer_params(**fields)))
    (loose,) = check(seq, TARGETS, targets, limit, loops=True, fields=fields, pair=base)
    (tight,) = check(seq, TARGETS, targets, limit, loops=True, fields=fields, pair=dict(base, **{limit: pp.PAIR_DEFAULTS[limit]}))
    assert pp.primers_of(loose) == alone and tight[0] >= 0 and tight[:12] != alone[:12]
    a, b = pc.oligo_of(alone[:6]), pp.reverse_complement(pc.oligo_of(alone[6:12]))
    value = abs(alone[2] - alone[8]) if limit == "max_tm_difference" else _value_of(limit, a, b)
    assert value > pp.PAIR_DEFAULTS[limit]
    # and the pair taken instead is within it
    a, b = pc.oligo_of(tight[:6]), pp.reverse_complement(pc.oligo_of(tight[6:12]))
    assert (tight[13] if limit == "max_tm_difference" else _value_of(limit, a, b)) <= pp.PAIR_DEFAULTS[limit]


def test_a_pair_that_is_not_the_two_best():
    (r,) = check(pc.clean_record(900, 1000), TARGETS, TARGETS[1:2], loops=True)
    assert r[0] >= 0 and (r[15], r[16]) == (0, 6)


def test_pairs_tried_and_none_admissible():
    (r,) = check(pc.clean_record(900, 1065), TARGETS, TARGETS[1:2], loops=True)
    assert r[:25] == NO_PAIR and r[29] == 40 and r[30] == 0 and r[27] >= 1 and r[28] >= 1


def test_non_default_parameters(records):
    seq, rows, targets = records["clean"]
    seq, targets = seq[:1500], targets[targets[:, 0] < 1400][:20]
    counts = {}
    for pair in [dict(shortlist=s) for s in (1, 3, 8)] + [dict({n: v}) for n in LIMITS for v in (0, 2, 32)] + [dict(max_tm_difference=v) for v in (0, 10, 2000)]:
        want = check(seq, rows, targets, pair=pair)
        counts[tuple(pair.items())[0]] = (sum(r[0] >= 0 for r in want), sum(r[27] + r[28] for r in want), sum(r[30] for r in want))
    # a tighter limit never lets more through
    for n in LIMITS:
        column = 2 if n.startswith("max_pair") else 1
        assert counts[(n, 0)][column] <= counts[(n, 2)][column] <= counts[(n, 32)][column] and counts[(n, 0)][column] < counts[(n, 32)][column]
    assert counts[("max_tm_difference", 0)][2] < counts[("max_tm_difference", 10)][2] < counts[("max_tm_difference", 2000)][2]
    assert counts[("shortlist", 1)][0] <= counts[("shortlist", 3)][0] <= counts[("shortlist", 8)][0]
    check(seq, rows, targets, fields=dict(SMALL, flank=60, min_length=2, max_length=32, opt_length=17, tm_max=2000), pair=dict(max_hairpin=5, max_self_any=8))


BED = "".join(f"rec one\t{s}\t{e}\tAC\t2\t{e - s}\t{(e - s) // 2}\t1.00\t+\tP\t{e - s}=\n" for s, e in ((60, 80), (0, 40), (290, 300), (150, 150)))


def test_the_text_byte_for_byte():
    seq = pc.clean_record(300, 3)
    rows = ribbit_amd.bed_intervals(BED).tolist()
    got = ribbit_amd.host_record_primer_pairs(seq, rows, rows, ribbit_amd.primer_params(**SMALL), ribbit_amd.primer_pair_params(**SMALL_PAIR))
    want = pp.pair_lines(BED, pp.record_primer_pairs(seq, rows, rows, pc.params(**SMALL), pp.pair_params(**SMALL_PAIR)))
    assert ribbit_amd.bed_primer_pairs_text(BED, got).decode() == want
    assert ribbit_amd.bed_primer_pairs_text(BED[:-1], got).decode() == want          # a last line without its newline counts
    lines = [line.split("\t") for line in want.splitlines()]
    assert all(len(line) == 32 and line[:11] == src.split("\t") for line, src in zip(lines, BED.splitlines()))
    # row 1 starts the record and row 2 ends it: a side without a candidate leaves no pair, and 18 columns of "."
    assert lines[1][11:29] == ["."] * 18 == lines[2][11:29] and lines[1][29] == "0" and lines[2][30] == "0" and lines[1][31] == "0"
    both = lines[0]
    assert int(both[19]) == int(both[16]) - int(both[11]) and seq[int(both[11]):int(both[12])].decode().upper() == both[13]
    assert seq[int(both[15]):int(both[16])].decode().upper() == both[17][::-1].translate(pc.COMPLEMENT)
    assert ribbit_amd.oligo_duplex(both[13], both[17]) == (int(both[21]), int(both[22])) and ribbit_amd.oligo_hairpin(both[17]) == int(both[28])
    assert both[20] == pc.tenths(abs(int(float(both[14]) * 10 + 0.5) - int(float(both[18]) * 10 + 0.5)))
    # the first nine of the 21 are what the primers' text writes for the same two primers
    as_primers = np.zeros(1, ribbit_amd.PRIMERS_DT)
    for name in ribbit_amd.PRIMERS_DT.names:
        as_primers[name] = got[name][:1]
    assert ribbit_amd.bed_primers_text(BED.splitlines()[0], as_primers).decode().split("\t")[11:20] == both[11:20]
    assert ribbit_amd.bed_primer_pairs_text("", got[:0]) == b""
    # the extreme values fit their columns
    big = np.zeros(1, ribbit_amd.PRIMER_PAIRS_DT)
    for name, value in zip(pp.FIELDS, (2**31 - 33, 32, 2000, 0, -1, -1, 2**31 - 33, 32, -15, 0, 0, 0, 0, 2015, 32, 7, 7) + (32,) * 8 + (2**31 - 1,) * 6 + (0,)):
        big[name] = value
    assert ribbit_amd.bed_primer_pairs_text("x", big).decode() == pp.pair_lines("x", pp.as_tuples(big))
    assert ribbit_amd.bed_primer_pairs_text("x", big).endswith(b"\t32\t201.5" + b"\t32" * 8 + b"\t2147483647" * 3 + b"\n")


def test_every_refusal_of_the_text():
    L = ribbit_amd.load_library()
    got = ribbit_amd.host_record_primer_pairs(pc.clean_record(300, 3), [], ribbit_amd.bed_intervals(BED).tolist(), ribbit_amd.primer_params(**SMALL),
                                              ribbit_amd.primer_pair_params(**SMALL_PAIR))
    assert got["left_start"][0] >= 0
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: the BED text has 4 lines, not the 3 of the rows"):
        ribbit_amd.bed_primer_pairs_text(BED, got[:3])
    for field, value in (("left_length", 0), ("left_length", 33), ("right_length", -1)):
        bad = got.copy()
        bad[field][0] = value
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: row 0: a primer of {value} bases, not 1 .. 32"):
            ribbit_amd.bed_primer_pairs_text(BED, bad)
    text, n = C.c_void_p(), C.c_size_t()
    f = L.ribbit_bed_primer_pairs_text
    assert f(b"x", 1, None, 1, C.byref(text), C.byref(n)) == -1 and f(None, 1, got.ctypes.data, 1, C.byref(text), C.byref(n)) == -1
    assert f(b"x", 1, got.ctypes.data, 1, None, C.byref(n)) == -1 and f(b"x", 1, got.ctypes.data, 1, C.byref(text), None) == -1
    assert b"null argument" in L.ribbit_hip_last_error()


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
    _dies(["--primer-pair-flank", "5"], "--primer-pair-flank needs --primer-pair-bed")
    _dies(["-i", "in.fa", "--primer-pair-flank=5"], "--primer-pair-flank needs --primer-pair-bed")
    # each flank belongs to its own output
    _dies(["--primer-pair-flank", "5", "--primer-bed", "b"], "--primer-pair-flank needs --primer-pair-bed")
    _dies(["--primer-flank", "5", "--primer-pair-bed", "b"], "--primer-flank needs --primer-bed")
    _dies(["--primer-pair-flank", "5", "--best-bed", "b"], "--primer-pair-flank needs --primer-pair-bed")
    # the first in the order of the eighteen
    _dies(["--primer-pair-flank", "5", "--primer-flank", "5"], "--primer-flank needs --primer-bed")
    _fails(["--primer-pair-bed", tmp_path / "missing" / "out", "--primer-pair-flank", "5"], "ERROR: Please specify an input fasta file!\n")
    assert not (tmp_path / "missing").exists()


@needs_tool
def test_cli_limit_values(tmp_path):
    out = tmp_path / "missing" / "out"
    for value in ("1001", "-1", "x", "10000", "00000", "1e3", "", "5 ", "+5"):
        _dies(["-i", "in.fa", "--primer-pair-bed", "b", "--primer-pair-flank", value], f"--primer-pair-flank wants a whole number of bases (0 .. 1000), got '{value}'")
    for value in ("0", "1000", "0200", "18"):
        _dies(["-i", tmp_path / "in.fa", "--primer-pair-bed", out, "--primer-pair-flank", value], f"--primer-pair-bed: cannot open '{out}' for writing")
    _dies(["-i", "in.fa", "--primer-pair-bed", "b", "--primer-pair-flank"], "the required argument for option '--primer-pair-flank' is missing")


@needs_tool
def test_cli_file_names():
    _dies(["--primer-pair-bed="], "--primer-pair-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-pair-bed", ""], "--primer-pair-bed wants a file name")
    _dies(["-i", "in.fa", "--primer-pair-bed"], "the required argument for option '--primer-pair-bed' is missing")
    _dies(["-i", "in.fa", "--primer-pair-bed", "x", "--primer-pair-any", "3"], "unrecognised option '--primer-pair-any'")
    _dies(["-i", "in.fa", "--primer-pairs-bed", "x"], "unrecognised option '--primer-pairs-bed'")


@needs_tool
def test_cli_the_file_is_opened_last(tmp_path):
    other = tmp_path / "other.bed"
    other.write_text("a\t1\t5\tgene\n")
    out = tmp_path / "missing" / "out"
    _dies(["-i", tmp_path / "in.fa", "--primer-pair-bed", out], f"--primer-pair-bed: cannot open '{out}' for writing")
    options = EARLIER_OUTPUTS + ["--primer-pair-bed"]
    assert len(options) == 18
    for bad in (16, 17):
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
    names = ["--primer-bed", "--primer-flank", "--primer-pair-bed", "--primer-pair-flank"]
    at = [r.stderr.index(f"\n  {name} arg ") for name in names]
    assert at == sorted(at)
    assert r.stderr[at[1]:at[2]].endswith("Default: 200") and r.stderr[at[3]:].rstrip("\n").endswith("Default: 200")
    assert "check_primers" in r.stderr[at[0]:at[1]] and "--primer-pair-bed is the checked form" in r.stderr[at[0]:at[1]]
    assert "21 columns" in r.stderr[at[2]:at[3]]
