"""GPU tests of the chunk contract at the cuts where a chunk's logic can go wrong: one oracle run per record, then many plans
checked against it.  A chunk is loaded with the tightest halos ribbit_hip_stage_calls_chunk accepts (2s+56 bases on the left,
4s+16 on the right, s = max_motif + 2), so a kernel whose true reach exceeded the claimed one would show here; its kept
calls, cursor bounds (each -1 or the largest end before it, and together moving a merge's cursors as the full call list would:
window_stage_contract.bounds_hold), tail_pend, flush calls, runs and run halves must be what tests/chunk_contract.py cuts out of the
oracle's lists of the whole record.  Cuts sit on calls' scan positions and group ends, on the edges of N blocks, inside long
N blocks and homopolymers, at the end of the record, and leave own ranges empty or one word long; the whole path (scan_part,
merge_parts, the BED) runs over the same cuts rounded to words, over a sharded fuzz, and pieces run at offsets near INT32_MAX."""
import functools

import numpy as np
import pytest

import ribbit_amd
from cases import _rand, edge_cases, large_motif_cases, simulated_cases, structured_cases
from chunk_contract import ANCHORED_SPAN, SUBST_SPAN, _chunk_calls, _chunk_runs, oracle_runs, spans
from fuzz import fuzz_case
from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle
from ribbit_amd import STAGE_ANCHORED, STAGE_SUBST, sharded
from window_stage_contract import bounds_hold

pytestmark = pytest.mark.gpu
INT32_MAX = 2**31 - 1
STAGES = ((STAGE_SUBST, "subst", LIST_SUBST, SUBST_SPAN), (STAGE_ANCHORED, "anchored", LIST_ANCHORED, ANCHORED_SPAN))
CALL_SAMPLE = 40           # calls per window stage whose position and group end become cuts
WHOLE_PATH_PLANS = 24      # word-aligned two-part plans per record through scan_part + merge_parts
BED_EVERY = 6              # of those, every BED_EVERY-th also through host_refine_bed


def _reach(m_hi):
    """(smallest left halo, smallest right halo) ribbit_hip_stage_calls_chunk accepts (api_chunks.cpp)"""
    s = m_hi + 2
    return 2 * s + 56, 4 * s + 16


def _records():
    pick = {c[0]: c for c in simulated_cases() + edge_cases() + structured_cases()}
    names = ["sim_cfg2_120k", "random_n_100k", "n_runs", "mostly_n", "homopolymer_40k_large_m", "dinucleotide_60k_sparse_mismatches"]
    return [pick[n] for n in names] + large_motif_cases()


RECORDS = {c[0]: c[1:] for c in _records()}
# for the pieces near INT32_MAX: sim_cfg2_120k with a dinucleotide run open at its end, so that both window stages make
# end-of-record calls (sim_cfg2_120k itself has none)
_sim = RECORDS["sim_cfg2_120k"]
OFFSET_RECORDS = {"sim_cfg2_120k_open_end": (_sim[0] + b"CA" * 100,) + _sim[1:], "M500_two_tiles": RECORDS["M500_two_tiles"]}
NO_BED = {"homopolymer_40k_large_m"}      # its oracle refinement alone takes ~12 s; test_sharded_gpu.py checks its BED


@functools.lru_cache(maxsize=None)
def _oracle(name):
    seq, m_lo, m_hi = {**RECORDS, **OFFSET_RECORDS}[name]
    with Oracle(seq, m_lo, m_hi) as o:
        runs = oracle_runs(o, m_lo, m_hi)
        o.run_all()
        return {"seq": seq, "m_lo": m_lo, "m_hi": m_hi, "L": len(seq), "runs": runs,
                "calls": {key: o.calls(lst) for _, key, lst, _ in STAGES},
                "want": {"perfect": o.seeds(LIST_PERFECT), "subst": o.seeds(LIST_SUBST), "anchored": o.seeds(LIST_ANCHORED),
                         "dispatch": o.dispatch(), "guard_hits": o.guard_hits()},
                "bed": None if name in NO_BED else o.refine_bed(name)}


@pytest.fixture(scope="module")
def scanner():
    made = {}

    def get(m_lo, m_hi):
        if (m_lo, m_hi) not in made:
            made[(m_lo, m_hi)] = ribbit_amd.Scanner(m_lo, m_hi)
        return made[(m_lo, m_hi)]
    yield get
    for sc in made.values():
        sc.close()


def _n_blocks(seq):
    n = np.frombuffer(seq, np.uint8)
    isn = ((n == ord("N")) | (n == ord("n"))).astype(np.int8)
    d = np.diff(np.concatenate(([0], isn, [0])))
    return [(int(a), int(b)) for a, b in zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1)]     # first and last base of each block


def _cuts(name):
    """cut positions in [0, L] derived from the oracle's output and the record (see the module doc)"""
    o = _oracle(name)
    L, rs = o["L"], np.random.RandomState(o["L"] + 7)
    cuts = {0, L, L // 32 * 32, max(0, L // 32 * 32 - 32)}
    for _, key, _, span in STAGES:
        c = o["calls"][key]
        c = c[c["pos"] < L]
        kept = c[(c["end"] - c["start"]) >= spans(c["mlen"], span)]
        for pool in (kept, c):                     # calls that reach a merge, and calls the length filter drops
            take = pool[np.sort(rs.choice(len(pool), min(len(pool), CALL_SAMPLE // 2), replace=False))] if len(pool) else pool
            for x in take:
                cuts.update((int(x["pos"]) - 1, int(x["pos"]), int(x["pos"]) + 1, int(x["end"]) + 7, int(x["end"]) + 8))
    blocks = _n_blocks(o["seq"])
    if len(blocks) > 30:
        blocks = [blocks[i] for i in np.sort(rs.choice(len(blocks), 30, replace=False))]
    for a, b in blocks:
        for p in (a, b):
            cuts.update((p - 8, p - 1, p, p + 1, p + 8))
        cuts.add((a + b) // 2)                     # inside the block (65 kb in mostly_n)
    if name.startswith("homopolymer"):
        cuts.update((700 + 20_000, 700 + 40_000 - 40))                # inside the 40-kb run
    return sorted(int(c) for c in cuts if 0 <= c <= L)


def _scan_chunk(sc, seq, L, m_hi, own_lo, own_hi, load_lo, load_hi, offset=0, record_length=None):
    """one chunk as a rank runs it; a stage that reports inexact makes the left halo four times longer, as scan_part does.
    offset / record_length: where the piece is put (default: its true place in this record)"""
    record_length = L if record_length is None else record_length
    grown = 0
    while True:
        sc.load_record(seq[load_lo:load_hi])
        lo_l, hi_l = own_lo - load_lo, own_hi - load_lo
        rec, halves = sc.scan_perfect_chunk(lo_l, hi_l, load_lo + offset)
        got = {"runs": np.array(rec[rec["term"] >= 0]), "halves": halves, "load_lo": load_lo}
        for st, key, _, _ in STAGES:
            got[key] = sc.stage_calls_chunk(st, lo_l, hi_l, load_lo + offset, record_length)
        if not (got["subst"]["inexact"] or got["anchored"]["inexact"]):
            got["grown"] = grown
            return got
        assert load_lo > 0, "a piece that starts where the record starts is exact by construction"
        load_lo = max(0, own_lo - 4 * (own_lo - load_lo))
        grown += 1


def _tight_plan(L, m_hi, own_lo, own_hi, align=1):
    left, right = _reach(m_hi)
    load_lo = max(0, own_lo - left) // align * align
    return int(own_lo), int(own_hi), int(load_lo), int(min(L, own_hi + right))


def _eq(a, b):
    return len(a) == len(b) and np.array_equal(np.asarray(a).view("<i4"), np.asarray(b).view("<i4"))


def _sorted_runs(r):
    return np.sort(r, order=["mlen", "start", "end", "term"])


def _check_chunk(o, got, own_lo, own_hi, where):
    L = o["L"]
    whole, halves = _chunk_runs(o["runs"], own_lo, own_hi)
    assert _eq(got["runs"], whole), f"{where}: perfect runs"
    assert _eq(_sorted_runs(got["halves"]), _sorted_runs(halves)), f"{where}: run halves"
    for _, key, _, span in STAGES:
        calls, seen, tail, flush = _chunk_calls(o["calls"][key], L, own_lo, own_hi, own_hi > L, span)
        g = got[key]
        assert _eq(g["calls"], calls), f"{where}: {key} calls"
        if g["pend"] is not None:
            assert np.all((g["pend"] == -1) | (g["pend"] == seen)), f"{where}: {key} pend"
        assert bounds_hold(g["calls"], g["pend"], seen), f"{where}: {key} cursor bounds"
        assert g["tail_pend"] == tail, f"{where}: {key} tail_pend"
        assert _eq(g["flush"], flush), f"{where}: {key} flush"


def _whole(sc, o):
    sc.load_record(o["seq"])
    L = o["L"]
    out = {key: sc.stage_calls_chunk(st, 0, L + 1, 0, L) for st, key, _, _ in STAGES}
    for _, key, _, span in STAGES:
        calls, seen, tail, flush = _chunk_calls(o["calls"][key], L, 0, L + 1, True, span)
        w = out[key]
        assert not w["inexact"] and _eq(w["calls"], calls) and w["tail_pend"] == tail and _eq(w["flush"], flush), key
        if w["pend"] is not None:
            assert np.all((w["pend"] == -1) | (w["pend"] == seen)), key
        assert bounds_hold(w["calls"], w["pend"], seen), f"{key} cursor bounds"
    return out


def _check_concat(chunks, whole, where):
    """the chunks' kept calls back to back are the whole record's; the bound the merge gives an edge call (its pend, or the
    earlier chunks' tail_pend) is the whole record's"""
    for _, key, _, _ in STAGES:
        w = whole[key]
        assert _eq(np.concatenate([c[key]["calls"] for c in chunks]), w["calls"]), f"{where}: {key} concatenated calls"
        assert _eq(np.concatenate([c[key]["flush"] for c in chunks]), w["flush"]), f"{where}: {key} concatenated flush"
        assert max(c[key]["tail_pend"] for c in chunks) == w["tail_pend"], f"{where}: {key} tail_pend"
        if w["pend"] is None:
            continue
        before, at = -1, 0
        for c in chunks:
            n = len(c[key]["calls"])
            wp = w["pend"][at:at + n]
            cp = c[key]["pend"] if c[key]["pend"] is not None else np.full(n, -1, np.int32)
            edge = wp != -1
            assert np.array_equal(np.maximum(cp, before)[edge], wp[edge]), f"{where}: {key} cursor bounds of edge calls"
            before = max(before, c[key]["tail_pend"])
            at += n


# ---- a. geometry limits --------------------------------------------------------------------------------------------

GEOMETRY_RANGES = [(2, 12), (2, 100), (2, 110), (90, 111), (100, 500), (500, 990)]


@pytest.mark.parametrize("m_lo,m_hi", GEOMETRY_RANGES, ids=[f"M{r[1]}" for r in GEOMETRY_RANGES])
def test_tightest_halos_are_accepted_and_one_base_less_is_rejected(scanner, m_lo, m_hi):
    sc = scanner(m_lo, m_hi)
    left, right = _reach(m_hi)
    seq = _rand(left + right + 3000, m_hi)
    n, off, rec_len = len(seq), 50_000, 50_000 + len(seq) + 9_000         # neither the first nor the last piece
    sc.load_record(seq)
    for st, key, _, _ in STAGES:
        sc.stage_calls_chunk(st, left, n - right, off, rec_len)
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"must reach {right} bases beyond"):
            sc.stage_calls_chunk(st, left, n - right + 1, off, rec_len)
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"must start at least {left} bases before"):
            sc.stage_calls_chunk(st, left - 1, n - right, off, rec_len)
        # the first piece needs no left halo, the last none on the right
        sc.stage_calls_chunk(st, 0, n - right, 0, rec_len)
        sc.stage_calls_chunk(st, left, n + 1, rec_len - n, rec_len)


# ---- b. adversarial cuts, call level ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(RECORDS))
def test_chunks_with_the_tightest_halos_keep_what_the_oracle_says(scanner, name):
    o = _oracle(name)
    seq, L, m_hi = o["seq"], o["L"], o["m_hi"]
    sc = scanner(o["m_lo"], m_hi)
    whole = _whole(sc, o)
    cuts = _cuts(name)
    for c in cuts:
        chunks = []
        for own_lo, own_hi in ((0, c), (c, L + 1)):
            plan = _tight_plan(L, m_hi, own_lo, own_hi)
            got = _scan_chunk(sc, seq, L, m_hi, *plan)
            _check_chunk(o, got, own_lo, own_hi, f"{name} cut {c} chunk {plan} (left halo grown {got['grown']}x)")
            chunks.append(got)
        _check_concat(chunks, whole, f"{name} cut {c}")
    # every cut at once, plus own ranges that are empty or one word long
    bounds = sorted(cuts[1:-1] + cuts[1:-1:7] + [c + 32 for c in cuts[3:-1:11] if c + 32 < L])
    bounds = [0] + bounds + [L, L + 1]                          # the last chunk owns the end-of-record calls only
    chunks = []
    for own_lo, own_hi in zip(bounds[:-1], bounds[1:]):
        plan = _tight_plan(L, m_hi, own_lo, own_hi)
        got = _scan_chunk(sc, seq, L, m_hi, *plan)
        _check_chunk(o, got, own_lo, own_hi, f"{name} many-part plan, chunk {plan}")
        chunks.append(got)
    assert any(a == b for a, b in zip(bounds[:-1], bounds[1:])) or len(cuts) < 4
    _check_concat(chunks, whole, f"{name} many-part plan ({len(chunks)} chunks)")
    if name == "mostly_n":
        assert max(c["grown"] for c in chunks) >= 1, "a cut inside the 65-kb N block must need a longer left halo"


# ---- c. adversarial cuts, whole path --------------------------------------------------------------------------------

def _merge_and_check(o, parts, where, bed=False, name="seq"):
    m_lo, m_hi, L = o["m_lo"], o["m_hi"], o["L"]
    got = sharded.merge_parts(m_lo, m_hi, L, parts)
    for k in ("perfect", "subst", "anchored", "dispatch"):
        assert _eq(got[k], o["want"][k]), f"{where}: {k}"
    assert got["guard_hits"] == o["want"]["guard_hits"], f"{where}: guard hits"
    if bed:
        hi, lo, brk, xa, stride = got["planes"]
        assert ribbit_amd.host_refine_bed(m_lo, m_hi, o["seq"], xa, stride, got["dispatch"], name) == o["bed"], f"{where}: BED"


@pytest.mark.parametrize("name", list(RECORDS))
def test_word_aligned_cuts_through_the_whole_path_match_the_oracle(scanner, name):
    o = _oracle(name)
    seq, L, m_hi = o["seq"], o["L"], o["m_hi"]
    sc = scanner(o["m_lo"], m_hi)
    cuts = sorted({c // 32 * 32 for c in _cuts(name)})
    rs = np.random.RandomState(L)
    pick = cuts if len(cuts) <= WHOLE_PATH_PLANS else [cuts[i] for i in np.sort(rs.choice(len(cuts), WHOLE_PATH_PLANS, replace=False))]
    for i, c in enumerate(pick):
        plans = [_tight_plan(L, m_hi, 0, c, 32), _tight_plan(L, m_hi, c, L + 1, 32)]
        parts = [sharded.scan_part(sc, seq, p) for p in plans]
        _merge_and_check(o, parts, f"{name} plan {plans}", bed=o["bed"] is not None and i % BED_EVERY == 0, name=name)
    bounds = [0] + cuts[1:] + [L + 1] if cuts and cuts[0] == 0 else [0] + cuts + [L + 1]
    plans = [_tight_plan(L, m_hi, a, b, 32) for a, b in zip(bounds[:-1], bounds[1:])]
    parts = [sharded.scan_part(sc, seq, p) for p in plans]
    _merge_and_check(o, parts, f"{name} many-part plan {plans}", bed=o["bed"] is not None, name=name)


# ---- d. sharded fuzz ------------------------------------------------------------------------------------------------

def _fuzz_seeds(first=9000, total=120, large=40):
    """a fixed block of fuzz seeds, at least `large` of them with m_hi > 100 (fuzz styles 8 and 9)"""
    out, n_large = [], 0
    seed = first
    while len(out) < total:
        seq, _, m_hi = fuzz_case(seed)
        if len(seq) >= 64 and (m_hi > 100 or len(out) - n_large < total - large):
            out.append(seed)
            n_large += m_hi > 100
        seed += 1
    return out


FUZZ_SEEDS = _fuzz_seeds()


@pytest.mark.parametrize("block", range(4))
def test_sharded_fuzz_matches_the_oracle(block):
    for seed in FUZZ_SEEDS[block::4]:
        seq, m_lo, m_hi = fuzz_case(seed)
        L = len(seq)
        with Oracle(seq, m_lo, m_hi) as o:
            o.run_all()
            want = {"perfect": o.seeds(LIST_PERFECT), "subst": o.seeds(LIST_SUBST), "anchored": o.seeds(LIST_ANCHORED),
                    "dispatch": o.dispatch(), "guard_hits": o.guard_hits()}
            bed = o.refine_bed(f"fuzz{seed}")
        rs = np.random.RandomState(seed)
        nparts = int(rs.randint(2, 10))
        cuts = sorted(int(c) * 32 for c in rs.randint(0, L // 32 + 1, size=nparts - 1))
        bounds = [0] + cuts + [L + 1]
        s = m_hi + 2
        plans = []
        for own_lo, own_hi in zip(bounds[:-1], bounds[1:]):
            left = int(rs.randint(2 * s + 56, 2 * s + 64 + 4096 + 1))
            right = int(rs.randint(4 * s + 16, 4 * s + 64 + 1))
            plans.append((own_lo, own_hi, max(0, own_lo - left) // 32 * 32, min(L, own_hi + right)))
        with ribbit_amd.Scanner(m_lo, m_hi) as sc:
            parts = [sharded.scan_part(sc, seq, p) for p in plans]
        _merge_and_check({"m_lo": m_lo, "m_hi": m_hi, "L": L, "seq": seq, "want": want, "bed": bed}, parts,
                         f"fuzz seed {seed} (-m {m_lo} -M {m_hi}, {L} bases), plan {plans}", bed=True, name=f"fuzz{seed}")


def test_the_fuzz_block_reaches_large_motif_ranges():
    assert len(set(FUZZ_SEEDS)) == 120 and sum(fuzz_case(s)[2] > 100 for s in FUZZ_SEEDS) >= 40


# ---- e. large offsets -----------------------------------------------------------------------------------------------

def _shifted(a, d):
    """a chunk's result moved d bases to the right: every coordinate but the -1 place holders"""
    out = {"runs": a["runs"].copy(), "halves": a["halves"].copy()}
    for k in ("runs", "halves"):
        for f in ("start", "end"):
            v = out[k][f]
            v[v != -1] += d
    for _, key, _, _ in STAGES:
        x = a[key]
        y = {"calls": x["calls"].copy(), "flush": x["flush"].copy(), "pend": None if x["pend"] is None else x["pend"].copy(),
             "tail_pend": x["tail_pend"] + d if x["tail_pend"] != -1 else -1}
        for k in ("calls", "flush"):
            for f in ("pos", "start", "end"):
                y[k][f] += d
        if y["pend"] is not None:
            y["pend"][y["pend"] != -1] += d
        out[key] = y
    return out


def _same_chunk(a, b, where):
    assert _eq(a["runs"], b["runs"]) and _eq(a["halves"], b["halves"]), f"{where}: runs"
    for _, key, _, _ in STAGES:
        x, y = a[key], b[key]
        assert _eq(x["calls"], y["calls"]) and _eq(x["flush"], y["flush"]), f"{where}: {key} calls"
        assert (x["pend"] is None) == (y["pend"] is None), f"{where}: {key} pend"
        assert x["pend"] is None or np.array_equal(x["pend"], y["pend"]), f"{where}: {key} pend"
        assert x["tail_pend"] == y["tail_pend"], f"{where}: {key} tail_pend"


@pytest.mark.parametrize("name", list(OFFSET_RECORDS))
def test_pieces_near_int32_max_are_the_same_pieces_shifted(scanner, name):
    o = _oracle(name)
    seq, L, m_hi = o["seq"], o["L"], o["m_hi"]
    sc = scanner(o["m_lo"], m_hi)
    left, right = _reach(m_hi)
    for own_lo, own_hi in ((L // 3 + 5, 2 * L // 3 + 3), (2 * L // 3 + 3, L + 1)):
        _, _, load_lo, load_hi = _tight_plan(L, m_hi, own_lo, own_hi)
        load_lo = max(0, load_lo - 8192)                         # room for the groups that straddle the cut: no retry here
        at = _scan_chunk(sc, seq, L, m_hi, own_lo, own_hi, load_lo, load_hi)
        load_lo = at["load_lo"]
        _check_chunk(o, at, own_lo, own_hi, f"{name} own [{own_lo}, {own_hi})")
        # a middle piece ends 3 kb before the end of a record of INT32_MAX bases; the last one ends where that record ends
        last = own_hi > L
        d = INT32_MAX - L if last else INT32_MAX - 3000 - load_hi
        far = _scan_chunk(sc, seq, L, m_hi, own_lo, own_hi, load_lo, load_hi, offset=d, record_length=INT32_MAX)
        assert far["grown"] == 0
        _same_chunk(far, _shifted(at, d), f"{name} own [{own_lo}, {own_hi}) moved by {d}")
        if last:
            for _, key, _, _ in STAGES:
                assert len(far[key]["flush"]) > 0 or name == "M500_two_tiles", key
                assert np.all(far[key]["flush"]["pos"] == INT32_MAX), key
    # one base more is not a record this API can address
    sc.load_record(seq[L - 5000:])
    for st, _, _, _ in STAGES:
        with pytest.raises(ribbit_amd.RibbitHipError, match="geometry"):
            sc.stage_calls_chunk(st, 2 * left, 5001, INT32_MAX + 1 - 5000, INT32_MAX + 1)
