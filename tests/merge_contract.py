"""The first parallel pass of the anchored stage's merge, range by range, as a contract: constructed seed lists, composed planes
and calls at the interface of ribbit_hip_debug_merge_ranges, what every range must leave behind, and the paths each case exists to
reach.  tests/test_merge_ranges.py (CPU) and tests/test_merge_ranges_gpu.py hand the cases to the host workers and to the lanes.

Plain Python over tests/pyref.py's AnchoredMerge (the second restatement of addSeedToSeedPositionsAnchored and mergeAllLists);
nothing here is derived from the kernel.  What a range is, is the host's definition (ribbit_amd/csrc/parallel_merge.h): the kept
calls between two cuts, merged into a list of its own that starts with a sentinel (-1, -1, 0, N) for every range but the first,
from the cursors the preparation computed, against the perfect and substitution lists as they stood before the stage.  The cuts,
the first call of every range and the start cursors are the host preparation's (the `prep` arguments below: the dict that
ribbit_amd.debug_merge_ranges returns); the reference merges each range ON ITS OWN from them, as a run with only_range does.

A range's predicted status comes from the sizes pyref reached (AnchoredMerge.peaks) and the caps the library reports:
more perfect-plus-substitution candidates than ps_cap + ps_spill, more candidates than cand_cap + cand_spill, more factor or
non-factor children than child_cap, or more keys in the factor coverage table than cov_cap, is `scratch_full`; everything else 0.

REQUIRED_TAGS lists, independently of the cases, every path the cases together must reach in a range that is merged with status 0.

Lists must hold the types their stage makes (P and N in the perfect list; S, Q and N in the substitution list).  The reference
retires a candidate in the list that the candidate's TYPE names: a seed typed for the other list is never retired, and a rule
that retires and starts the call again (:268, :285, :376) then repeats without end -- in pyref (RecursionError), on the host
workers, and on a lane until AM_RUNAWAY.  The entry point refuses such lists.

Left out, as the issue says: AM_RUNAWAY (2^20 rounds of one call) and AM_BAD_PLANE (a motif size outside the planes: the entry
point refuses such input, since the host would read planes that are not there).
"""
import functools
import random

import numpy as np

import pyref
from pyref import RANK_A, RANK_C, RANK_N, RANK_P, RANK_Q, RANK_S

def library_caps():
    """the kernel's caps as the library reports them (no GPU: any run on the host workers returns them)"""
    import ribbit_amd
    xa, stride = ribbit_amd.pack_bit_planes([np.ones(3000, np.uint8)], 3000)
    return ribbit_amd.debug_merge_ranges(None, 4, 4, 3000, [], [], [(140, 4, 100, 140), (2040, 4, 2000, 2040)], xa, stride, where=ribbit_amd.MERGE_ON_HOST)["caps"]


SENTINEL = [-1, -1, 0, RANK_N]


class Case:
    """lists: (start, end, motif, type) sorted by start; calls: (pos, motif, start, end) in the scanner's order; plane_bits: motif ->
    one byte per base (missing motifs: all ones); tags: what the case exists to reach, in some range (see ref_range)"""

    def __init__(self, name, m_lo, m_hi, length, perfect, subst, calls, plane_bits=None, tags=(), calls_per_range=1, max_passes=0):
        self.name, self.m_lo, self.m_hi, self.length = name, m_lo, m_hi, length
        self.perfect, self.subst, self.calls = sorted(perfect), sorted(subst), list(calls)
        self.plane_bits = plane_bits or {}
        self.tags = tuple(tags)
        self.calls_per_range, self.max_passes = calls_per_range, max_passes
        ones = np.ones(length, np.uint8)
        self.planes = {m: self.plane_bits.get(m, ones) for m in range(m_lo, m_hi + 1)}

    def __repr__(self):
        return f"Case({self.name})"

    def kept(self):
        """the stage's filter and cursor bounds (compact_full of parallel_merge.cpp): (calls that pass the length filter,
        pend = the largest end of ANY earlier call, or -1), the flush calls (pos == length) apart"""
        kept, pend, seen = [], [], -1
        for pos, m, start, end in self.calls:
            if pos == self.length:
                break
            if end - start >= pyref.anchored_cutoff(m):
                kept.append((pos, m, start, end))
                pend.append(seen)
            seen = max(seen, end)
        return kept, pend


def advance(lst, frm, seed_end):
    """the cursor loop (seed_lists.h: advance_cursor)"""
    while frm < len(lst) and lst[frm][0] <= seed_end and frm != len(lst) - 1:
        frm += 1
    return frm


def ref_range(case, prep, k):
    """range k merged on its own by pyref, from the preparation's first[] and start cursors -> dict: own (without the sentinel),
    guards, cursor, undo (sorted (list, index, old type)), heads (the writes to list heads, logged and not made, as a worker
    does: sorted (list, index, start, end, motif, type)), peaks (the largest sizes over the range's calls), met (pyref's tags and
    the cursor tags below)"""
    kept, pend = case.kept()
    am = pyref.AnchoredMerge(case.perfect, case.subst, case.planes, case.length)
    am.head_write_log = []
    if k > 0:
        am.A.append(list(SENTINEL))
    cur = tuple(int(v) for v in prep["cursors0"][k])
    pending = -1
    for i in range(int(prep["first"][k]), int(prep["first"][k + 1])):
        _, m, start, end = kept[i]
        pending = max(pending, pend[i])
        if pending >= 0:
            moved = (advance(am.P, cur[0], pending), advance(am.S, cur[1], pending))
            if moved != cur:
                am.met["calls that only moved the cursors, folded into one advance"] += 1
            cur, pending = moved, -1
        cur = am.add(start, end, m, cur, RANK_A)
    for lst, at in ((am.P, cur[0]), (am.S, cur[1])):
        if lst and at == len(lst) - 1:
            am.met["cursor held at the last entry"] += 1
    undo = sorted((which, i, int(before[i][3])) for which, before, after in ((0, case.perfect, am.P), (1, case.subst, am.S))
                  for i in range(len(before)) if before[i][3] != after[i][3])
    peaks = {key: max((p[key] for p in am.peaks), default=0) for key in ("ps", "cands", "factor", "nonfactor", "sizes")}
    return {"own": [tuple(s) for s in am.A[1 if k > 0 else 0:]], "guards": am.guards, "cursor": cur, "undo": undo, "peaks": peaks, "met": am.met,
            "heads": sorted(am.head_write_log)}


def predicted_status(peaks, caps):
    full = (peaks["ps"] > caps["ps_cap"] + caps["ps_spill"] or peaks["cands"] > caps["cand_cap"] + caps["cand_spill"] or
            peaks["factor"] > caps["child_cap"] or peaks["nonfactor"] > caps["child_cap"] or peaks["sizes"] > caps["cov_cap"])
    return caps["scratch_full"] if full else 0


def ref_full(case):
    """the whole stage in call order -> (perfect, subst, anchored as lists of tuples, guards)"""
    am = pyref.AnchoredMerge(case.perfect, case.subst, case.planes, case.length).run(case.calls)
    return [tuple(s) for s in am.P], [tuple(s) for s in am.S], [tuple(s) for s in am.A], am.guards


# --------------------------------------------------------------------------------------------------------------------- the cases
# Every locus is a group of calls and seeds around one place, far from the next, so that the preparation cuts between loci (a cut
# needs a position that no call and no seed covers).  Inside a locus the calls interact, so a locus is one range -- or several,
# where its calls happen to leave a gap.

def _random_planes(rng, length, motifs, density=0.5):
    return {m: (rng.random(length) < density).astype(np.uint8) for m in motifs}


def _rule_loci(name, seed, n_loci, motifs, m_lo, m_hi, spacing, span, tags):
    """n_loci random loci of one to three calls and zero to five seeds of either list, intervals in every relation to each other
    (identical, nested, around, overlapping on either side, apart, tiny seeds inside), motif sizes from `motifs` (divisors,
    multiples and strangers of each other), seed types P and N in the perfect list, S, Q and N in the substitution list; some
    calls too short for the stage's filter.  Planes: random bits, so that every count of a nested-seed test depends on the exact
    interval.  (A seed typed for the other list is never retired by the reference's rules and its call restarts without end:
    the entry point refuses such lists, tests/test_merge_ranges.py.)"""
    rnd = random.Random(seed)
    rng = np.random.default_rng(seed)
    length = spacing * (n_loci + 2)
    perfect, subst, calls = [], [], []
    for j in range(n_loci):
        base = spacing * (j + 1)
        m0 = rnd.choice(motifs)
        lo = base + rnd.randrange(0, span // 4)
        hi = lo + max(pyref.anchored_cutoff(m0) + rnd.randrange(0, 4 * m0 + 8), rnd.randrange(10, span // 2))
        anchor = (lo, hi)

        def related(kind):
            s, e = anchor
            n = e - s
            d1, d2 = rnd.randrange(1, max(2, n // 2)), rnd.randrange(1, max(2, n // 2))
            if kind == "same":
                return s, e
            if kind == "inside":
                return s + d1 // 2, max(s + d1 // 2 + 1, e - d2 // 2)
            if kind == "around":
                return max(base - span // 4, s - d1), e + d2
            if kind == "left":
                return max(base - span // 4, s - d1), e - d2 // 2 - 1
            if kind == "right":
                return s + d1 // 2 + 1, e + d2
            if kind == "tiny":                          # a short seed inside: the children of :268 / :312
                t = s + rnd.randrange(0, max(1, n - 4))
                return t, min(e, t + rnd.randrange(1, 6))
            return e + rnd.randrange(1, 12), e + rnd.randrange(14, 40)      # apart, to the right

        kinds = ("same", "inside", "around", "left", "right", "tiny", "tiny", "tiny", "apart")
        for lst, types in ((perfect, (RANK_P, RANK_P, RANK_P, RANK_N)), (subst, (RANK_S, RANK_S, RANK_Q, RANK_Q, RANK_N))):
            only_tiny = rnd.random() < 0.3
            for _ in range(rnd.choice((0, 0, 1, 1, 2, 3, 4, 5))):
                m = rnd.choice(motifs) if rnd.random() < 0.7 else m0
                s, e = related("tiny" if only_tiny else rnd.choice(kinds))
                lst.append((s, e, m, rnd.choice(types)))
        for c in range(rnd.choice((1, 2, 2, 3, 3))):
            m = m0 if c == 0 or rnd.random() < 0.45 else rnd.choice(motifs)
            s, e = anchor if c == 0 else related(rnd.choice(kinds[:5] + ("same", "around", "inside")))
            if rnd.random() < 0.85 and e - s < pyref.anchored_cutoff(m):      # long enough for the filter, most of them
                e = s + pyref.anchored_cutoff(m) + rnd.randrange(0, 3)
            calls.append((e, m, s, e))
    calls.append((length - 40, motifs[0], length - 60, length - 40))      # the far-away isolated call
    return Case(name, m_lo, m_hi, length, perfect, subst, calls, _random_planes(rng, length, range(m_lo, m_hi + 1)), tags)


SMALL = (2, 3, 4, 5, 6, 8, 9, 12, 16, 18, 24)
TOP = (330, 495, 660, 989, 990)


def _chain_locus(base, primes, perfect, calls, early=0, merge_at=()):
    """staggered calls of pairwise unrelated motif sizes: partial overlaps of anchored seeds with different motifs do nothing, so
    call i walks back over the i entries before it, all of which reach it.  early: that many calls first, ending before the others
    start (a retired perfect seed covers the gap, so that no cut falls there): the walk of every later call ends at the last of them,
    inside a batch.  merge_at: indices whose call repeats the motif before it: the two join (:398) and leave a retired entry behind."""
    at = base
    for i in range(early):
        calls.append((at + 40, 7 + 2 * i, at, at + 40))
        at += 3
    if early:
        perfect.append((at + 30, at + 60, 2, RANK_N))
        at += 50
    for i, m in enumerate(primes):
        if i in merge_at:
            m = primes[i - 1]
        calls.append((at + 4 * i + 160, m, at + 4 * i, at + 4 * i + 160))


PRIMES = (7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79)


def walks_case():
    """(c) the batched walk over the range's own list: 1 .. 19 entries (so 7, 8, 9, 16 and 17, a batch being eight), in range 0
    (the walk ends at index -1) and in a later range (at the sentinel), with retired entries among them, and ending inside a batch
    at an entry that lies before the call."""
    perfect, calls = [], []
    _chain_locus(1000, PRIMES, perfect, calls)
    _chain_locus(4000, PRIMES, perfect, calls, merge_at=(3, 9))
    _chain_locus(7000, PRIMES[:14], perfect, calls, early=3)
    length = 10000
    calls.append((length - 40, 7, length - 60, length - 40))
    rng = np.random.default_rng(5)
    tags = tuple(f"own walk {n}" for n in (7, 8, 9, 16, 17)) + ("own walk 9, retired among them", "own walk 17, retired among them",
                                                                  "own walk ends by an entry before the seed", "own walk ends at index -1",
                                                                  "own walk ends by an entry before the seed (the sentinel)")
    return Case("walks", 2, 80, length, perfect, [], calls, _random_planes(rng, length, range(2, 81)), tags, calls_per_range=1)


def _dense_locus(base, kind, n, perfect, subst, calls):
    """one call and n seeds that all become candidates of it and change nothing:
    ps        perfect and substitution seeds that overlap the call from the left, motif twice the call's (:376, related sizes)
    factor    tiny perfect seeds inside, motif 2 under a call of motif 60 (:268, too short to take over: factor children)
    nonfactor the same under a call of motif 61 (:312)"""
    if kind == "ps":
        for j in range(n):
            (perfect if j % 3 else subst).append((base + j, base + 300 + j, 6, RANK_P if j % 3 else RANK_S))
        calls.append((base + 900, 3, base + 290, base + 900))
    else:
        for j in range(n):
            perfect.append((base + 4 * j, base + 4 * j + 3, 2, RANK_P))
        calls.append((base + 4 * n + 60, 60 if kind == "factor" else 61, base, base + 4 * n + 60))


def caps_case(repeats=1, name="caps"):
    """(f) one below, at and one above every cap (the far end of the candidate spill: cand_spill_case), each in a range of its own,
    ordinary ranges between them.  The list heads hold
    seeds of 70 different motif sizes, retired: the factor coverage reads them by loop counter, which is what fills its table."""
    caps = library_caps()
    perfect, subst, calls = [], [], []
    for j in range(70):
        perfect.append((10 + 3 * j, 12 + 3 * j, 2 + j, RANK_N))
    base, wanted = 2000, []
    ps_end, child, cov = caps["ps_cap"] + caps["ps_spill"], caps["child_cap"], caps["cov_cap"]
    # (a call also meets the next seed of either list at its cursors, where there is one: one or two candidates more than the
    # locus holds, so a size more than the three around each cap; the test asks for cap - 1, cap and cap + 1 among pyref's peaks)
    for kind, sizes in repeats * (("ps", tuple(t + d - 2 for t in (caps["ps_cap"], caps["cand_cap"], ps_end) for d in (-1, 0, 1, 2))),
                        ("factor", (cov - 1, cov, cov + 1, child - 1, child, child + 1)),
                        ("nonfactor", (child - 1, child, child + 1))):
        for n in sizes:
            _dense_locus(base, kind, n, perfect, subst, calls)
            if kind != "ps":
                wanted.append((kind, n))
            base += 2000
            calls.append((base - 940, 5, base - 1000, base - 940))      # an ordinary range between two dense ones
    wanted += [("ps", t + d) for t in (caps["ps_cap"], caps["cand_cap"], ps_end) for d in (-1, 0, 1)]
    length = base + 1000
    calls.append((length - 40, 7, length - 60, length - 40))
    rng = np.random.default_rng(6)
    return Case(name, 2, 80, length, perfect, subst, calls, _random_planes(rng, length, range(2, 81)), ("by-counter index 63 or above",),
                calls_per_range=1), wanted


def no_subst_case():
    """the substitution list empty (the guard of merge_types.cpp:24 counts once per round), one perfect seed"""
    calls = [(140, 4, 100, 140), (150, 4, 100, 150), (1040, 6, 1000, 1040), (1960, 7, 1940, 1960)]
    return Case("no substitution seeds, one perfect seed", 2, 12, 2000, [(90, 120, 4, RANK_P)], [], calls, tags=("one perfect seed",))


def no_perfect_case():
    calls = [(140, 4, 100, 140), (150, 4, 100, 150), (1040, 6, 1000, 1040), (1960, 7, 1940, 1960)]
    return Case("no perfect seeds", 2, 12, 2000, [], [(90, 120, 4, RANK_S), (95, 130, 8, RANK_Q)], calls, tags=("no perfect seed",))


def clamp_case():
    """a call that reaches the record's end: clamped to length - motif (:529)"""
    length = 3000
    calls = [(140, 4, 100, 140), (1040, 6, 1000, 1040), (length - 1, 12, length - 80, length - 2)]
    return Case("clamp at the record's end", 2, 12, length, [(90, 120, 4, RANK_P)], [(95, 130, 8, RANK_S)], calls, tags=("clamped to the record's end",))


def plane_case():
    """(e) nested anchored seeds of unrelated motif sizes whose intervals start and end on word boundaries, lie inside one word and
    end at bit 31, on the planes of the smallest and the largest motif (random bits: a wrong mask changes a count)"""
    calls, base = [], 1024
    for s, e in ((0, 64), (32, 96), (3, 29), (40, 64), (5, 64), (32, 61), (1, 127), (64, 65 + 31)):
        for big, small in ((12, 11), (11, 12), (7, 12), (12, 7)):
            # the older seed around, the newer inside it (:257), then one around both (:323)
            calls.append((base + e + 32, big, base + s - 32 if s >= 32 else base, base + e + 32))
            calls.append((base + e, small, base + s, base + e))
            base += 1024
    length = base + 1024
    calls.append((length - 40, 7, length - 60, length - 40))
    rng = np.random.default_rng(8)
    return Case("plane reads", 7, 12, length, [(10, 20, 7, RANK_P)], [(12, 22, 8, RANK_S)], calls, _random_planes(rng, length, range(7, 13)),
                (":257 keep", ":257 drop", "plane read on motif 7", "plane read on motif 12", "plane read starts on a word boundary",
                 "plane read ends on a word boundary (bit 31)", "plane read inside one word", "plane read over three words or more"), calls_per_range=1)


def by_hand_case():
    """the rules that random loci rarely reach, one locus each, eight copies at different places (the nested-seed tests read random
    planes).  All anchored against anchored; a locus is a list of (motif, start, end) relative to its base."""
    loci = (
        ((2, 0, 100), (4, 10, 60)),                 # :241 not for a motif of 4
        ((4, 0, 100), (2, 10, 60)),                 # :246 not for an old motif of 4
        ((8, 0, 40), (2, 1, 40)),                   # :246 again: 39 + 2 reaches both the old motif and the old length
        ((24, 0, 100), (2, 10, 20)),                # :246 neither: 10 + 2 is short of 23 and of 100
        ((2, 50, 60), (24, 0, 200)),                # :323 / :332 not again: 10 + 2 is short of 22 and of 198
        ((5, 0, 60), (5, 55, 100)),                 # :398 the old seed as long, a long new seed, ten bases of overlap: False
        ((5, 0, 60), (5, 40, 100)),                 # ... twenty-five: True
        ((5, 0, 100), (5, 90, 104)),                # (too short for the filter: only moves the cursors)
        ((5, 20, 40), (5, 0, 30)), ((5, 30, 100), (5, 0, 40)), ((12, 30, 100), (12, 0, 32)), ((12, 0, 30), (12, 25, 100)),
        ((5, 0, 30), (5, 28, 100)), ((5, 80, 100), (5, 0, 82)), ((6, 70, 100), (6, 0, 74)), ((9, 0, 12), (9, 10, 40)), ((9, 30, 40), (9, 0, 33)),
    )
    calls, base = [], 1000
    for copy in range(8):
        for locus in loci:
            for m, s, e in locus:
                calls.append((base + e + copy, m, base + s + copy, base + e + copy))
            base += 1000
    length = base + 1000
    calls.append((length - 40, 7, length - 60, length - 40))
    rng = np.random.default_rng(21)
    tags = (":241 not for a motif of 4", ":246 not for an old motif of 4", ":246 again, by the length", ":246 neither", ":332 not again",
            ":398 old as long, long new seed: False", ":398 old as long, long new seed: True")
    return Case("rules by hand", 2, 24, length, [(10, 20, 7, RANK_P)], [(12, 22, 8, RANK_S)], calls, _random_planes(rng, length, range(2, 25)), tags)


def two_sizes_case():
    """ST_TAIL chooses the SMALLEST factor size whose coverage reaches 0.8, not the first it meets.  Two factor children under a call
    of motif 24, of sizes 3 and 2 in the order the call meets them (by descending end); the coverage sums are read off the list
    heads by loop counter: entry 0 (size 3, 90 + 3 long) and entry 1 (size 2, 90 + 2 long), both above 80 of the call's 100.  The
    call takes size 2, the second one it met."""
    perfect = [(10, 100, 3, RANK_N), (120, 210, 2, RANK_N), (5230, 5233, 2, RANK_P), (5240, 5244, 3, RANK_P)]
    subst = [(300, 310, 4, RANK_N)]
    calls = [(5300, 24, 5200, 5300), (8960, 7, 8940, 8960)]
    rng = np.random.default_rng(23)
    return Case("list heads, two sizes", 2, 24, 9000, perfect, subst, calls, _random_planes(rng, 9000, range(2, 25)),
                ("takes the smallest of several factor sizes", "takes a factor's motif size"))


def cand_spill_case():
    """(f) the far end of the candidate spill: cand_cap + cand_spill - 1, that many, and one more candidates for one call (the last:
    predicted scratch_full), with the perfect-plus-substitution candidates well inside their own spill.  A locus is k short calls
    of motif 5, twenty bases apart -- each ends before the next starts, so none of them walks back further than one entry; a
    retired perfect seed over the whole locus keeps the preparation from cutting between them -- and one call of motif 7 around
    them all, which meets every one of the k entries (:323) and 200 perfect and substitution seeds of motif 14 that end just
    inside its start (:376, related sizes: no action)."""
    caps = library_caps()
    end = caps["cand_cap"] + caps["cand_spill"]
    perfect, subst, calls, base = [], [], [], 1000
    for k in range(end - 202, end - 198):                 # (200 seeds and what the cursors add: the test finds end - 1, end, end + 1 among the peaks)
        b = base + 500
        perfect.append((b - 450, b + 20 * k + 60, 2, RANK_N))
        for j in range(200):
            (perfect if j % 2 else subst).append((b - 400 + j, b - 5 + j % 5, 14, RANK_P if j % 2 else RANK_S))
        for i in range(k):
            calls.append((b + 20 * i + 12, 5, b + 20 * i, b + 20 * i + 12))
        calls.append((b + 20 * k + 50, 7, b - 5, b + 20 * k + 50))
        base = b + 20 * k + 1000
    length = base + 1000
    calls.append((length - 40, 7, length - 60, length - 40))
    rng = np.random.default_rng(24)
    return Case("cand spill end", 2, 14, length, perfect, subst, calls, _random_planes(rng, length, range(2, 15)), (":323 kept, no factor",))


def heads_case():
    """ST_TAIL's factor coverage reads and writes the HEADS of the lists by loop counter.  One factor child under a call of motif 24:
    the coverage is that of perfect entry 0, 85 + 2 of the call's 100, so the call takes the motif 2 and entry 0 (motif 2) is
    written -- logged.  First locus: entry 0 is live and in the call's range (a retired substitution seed covers the gap between
    them): the write would change its type, e[7] = 1.  Second locus, far away: the same write from another range, e[7] = 0.
    Third: a child typed P counted beyond the perfect list's end (guard)."""
    perfect = [(1000, 1085, 2, RANK_P), (1230, 1233, 2, RANK_P), (5230, 5233, 2, RANK_P)]
    subst = [(1080, 1210, 3, RANK_N), (9010, 9013, 2, RANK_S), (9020, 9023, 2, RANK_S), (9030, 9033, 2, RANK_S), (9040, 9043, 2, RANK_S)]
    calls = [(1300, 24, 1200, 1300), (5300, 24, 5200, 5300), (9100, 7, 9000, 9100), (11960, 7, 11940, 11960)]
    rng = np.random.default_rng(22)
    tags = ("takes a factor's motif size", "list-head write", ":268 factor child", "head write changed_then 1", "head write changed_then 0")
    return Case("list heads", 2, 24, 12000, perfect, subst, calls, _random_planes(rng, 12000, range(2, 25)), tags)


def short_lists_case():
    """children counted beyond a list's end: one perfect seed and three substitution seeds inside a call of an unrelated motif, all
    non-factor children; the perfect one is not the first, so its counter is past the perfect list's only entry (guard)"""
    perfect = [(1010, 1013, 2, RANK_P)]
    subst = [(1020, 1023, 2, RANK_S), (1030, 1033, 2, RANK_Q), (1040, 1043, 2, RANK_S)]
    calls = [(1100, 7, 1000, 1100), (2960, 7, 2940, 2960)]
    return Case("short lists", 2, 12, 3000, perfect, subst, calls, tags=("by-counter index beyond the list", ":312 non-factor child",
                                                                            "merged-type seed: values of the step before"))


def cursor_bounds_case():
    """(d) a call too short for the filter that ends further right than the kept call before it: its end reaches the next kept
    call as that call's cursor bound (pend), and both cursors move over the seeds in between before the call's own round starts"""
    perfect = [(990, 995, 2, RANK_N), (1120, 1123, 2, RANK_P), (1140, 1143, 2, RANK_P), (2500, 2503, 2, RANK_P)]
    subst = [(991, 996, 2, RANK_N), (1125, 1128, 2, RANK_S), (2600, 2603, 2, RANK_S)]
    calls = [(1100, 7, 1000, 1100), (1156, 7, 1150, 1155), (1101, 11, 1050, 1101), (2960, 7, 2940, 2960)]
    return Case("cursor bounds", 2, 12, 3000, perfect, subst, calls, tags=("calls that only moved the cursors, folded into one advance",))


# What the cases together must reach, in ranges that are predicted to fit (and that a lane then merges with status 0): written here
# independently of the cases, by the issue's sections.  tests/test_merge_ranges.py holds pyref to it, tests/test_merge_ranges_gpu.py
# the lanes.
REQUIRED_TAGS = (
    # a. every candidate rule of ST_CANDS
    ":203", ":205", ":208", ":215 returns", ":215 retires", ":215 goes on", ":231 higher type returns", ":231 C inside A",
    ":241 returns", ":241 not for a motif of 4", ":246", ":246 not for an old motif of 4", ":246 again, by the motif", ":246 again, by the length",
    ":246 neither", ":257 keep", ":257 drop", ":268 again, by the motif", ":268 again, by the length", ":268 factor child",
    ":285 again", ":285 no action", ":301 again", ":301 no action", ":312 non-factor child", ":319", ":323 equal sizes", ":323 nested test lost",
    ":323 kept, no factor", ":332 again", ":332 not again",
    ":351 old seed first, reach with its motif", ":351 old seed first, reach its end", ":351 new seed first, reach with its motif",
    ":351 new seed first, reach its end", ":351 old seed first, overlap to the new end", ":351 old seed first, overlap to the reach",
    ":351 new seed first, overlap to the old end", ":351 new seed first, overlap to the reach",
    ":376 merge", ":376 return", ":376 unrelated sizes, small overlap", ":376 related sizes, no action",
    ":398 old as long, long new seed: True", ":398 old as long, long new seed: False", ":398 old as long, short new seed: True",
    ":398 old shorter but long: True", ":398 old shorter but long: False", ":398 old shorter, short new seed: True",
    ":268 with a motif near the top", ":285 with a motif near the top", ":301 with a motif near the top", ":376 with a motif near the top",
    "plane read on motif 989", "plane read on motif 330", "plane read on motif 495", "added again by a nested call",
    # b. ST_TAIL
    "non-factor coverage: up to the start before", "non-factor coverage: the child with its motif", "non-factor coverage: up to the seed's end",
    "rejected: covered by other motif sizes", "non-factor coverage at or below half", "merged-type seed: values of the step before",
    "by-counter index beyond the list", "by-counter index 63 or above", "factor coverage: up to the start before",
    "factor coverage: the child with its motif", "factor coverage: up to the seed's end", "takes a factor's motif size",
    "takes the smallest of several factor sizes", "no factor size covers enough", "list-head write", "head write changed_then 0", "head write changed_then 1", "clamped to the record's end",
    # c. the batched walks
    "own walk 7", "own walk 8", "own walk 9", "own walk 16", "own walk 17", "own walk 9, retired among them", "own walk 17, retired among them",
    "own walk ends by an entry before the seed", "own walk ends by an entry before the seed (the sentinel)", "own walk ends at index -1",
    "phase 1 perfect alone 3", "phase 1 perfect alone 4", "phase 1 perfect alone 5", "phase 1 substitution alone 3", "phase 1 substitution alone 4",
    "phase 1 substitution alone 5", "phase 1 both open for 1 steps, then perfect alone", "phase 1 both open for 2 steps, then substitution alone",
    "phase 1 both open for 3 steps, then perfect alone", "phase 1 both open for 5 steps, then substitution alone",
    "no perfect seed", "one perfect seed",
    # d. cursors
    "calls that only moved the cursors, folded into one advance", "cursor held at the last entry",
    # e. plane reads
    "plane read starts on a word boundary", "plane read ends on a word boundary (bit 31)", "plane read inside one word",
    "plane read over three words or more", "plane read on motif 7", "plane read on motif 12",
)
# Not in the list, because the stage's own length filter rules them out (every anchored entry is at least 0.9 motif long, and a
# candidate that is met overlaps the call): the two ':398 ... short new seed: False' outcomes need an overlap below motif - 1 between
# two seeds of one motif that touch.  (f), (g) and (h) are sizes, lanes and budgets, not paths: tests/test_merge_ranges.py and
# tests/test_merge_ranges_gpu.py assert them directly.


@functools.lru_cache(maxsize=None)
def lanes_case():
    """(g) more than 130 ranges, dense ones that spill or overflow between ordinary ones all along: with one resident wavefront
    every lane takes several ranges, some of them after a range it had to give up"""
    return caps_case(repeats=4, name="lanes")[0]


@functools.lru_cache(maxsize=None)
def all_cases():
    caps, _ = caps_case()
    rules = _rule_loci("rules, small motifs", 14, 420, SMALL, 2, 24, 700, 240, ())
    other = _rule_loci("", 11, 420, SMALL, 2, 24, 700, 240, ())
    eight = Case("rules, eight calls to a range", 2, 24, other.length, other.perfect, other.subst, other.calls, other.plane_bits, (), calls_per_range=8)
    return (
        walks_case(), caps, no_subst_case(), no_perfect_case(), clamp_case(), plane_case(), rules, eight,
        _rule_loci("rules, motifs near the top", 12, 40, TOP, 329, 990, 9000, 2400, ()), by_hand_case(), heads_case(), short_lists_case(),
        cursor_bounds_case(), two_sizes_case(), cand_spill_case(), lanes_case(),
    )


def all_tags():
    """what the tests hold the cases to: the required list and whatever else a case names"""
    return tuple(dict.fromkeys(REQUIRED_TAGS + tuple(t for c in all_cases() for t in c.tags)))
