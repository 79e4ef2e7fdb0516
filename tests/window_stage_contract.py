"""The window stage's contract on constructed pass-streaks (tests/test_window_stage_contract.py without a GPU,
tests/test_window_stage_gpu.py on the kernels): what ribbit_hip_debug_window_calls must return for streaks made at will.

Nothing here comes from the kernels.  A record is bit planes (1 = the base matches its partner) and an N mask, both made up, not
derived from a sequence; its pass-streaks are pyevents.window_events on a stub that serves those planes; what must come out is cut
from the sequential call log, pyref.window_calls on the same planes (the literal per-position state machine), and the cursor
bounds from pystreaks.compact_bounds.  Only the record's bytes (`A`, `N` where the mask is set) and the streaks reach the GPU.

A window of 8 passes with at most `ALLOWED` zero bits, so in a plane of long stretches of ones
  * one zero alone fails no window; two zeros d <= 7 apart fail the 8 - d windows that hold both;
  * z >= 2 zeros in a row fail z + 5 windows: z = 2 is a gap of exactly 7 windows (the next streak joins), z = 3 one of 8 (it
    does not);
  * a single N at x leaves windows x - 7 .. x unevaluated: a streak it closes ends at x - 7 and the next one starts at x + 1 at
    the earliest, 8 behind it.  A gap of 7 after an N-closed streak therefore exists in no plane; 8 is the smallest.
An ordinary call is made 8 behind its end and ends 7 behind a streak, so position 16 is the first at which one can be made."""
import functools

import numpy as np

import pyevents
import pyref
import pystreaks
from chunk_contract import ANCHORED_SPAN, SUBST_SPAN
from ribbit_amd import RUN_DT

ALLOWED = 1                      # zero bits a passing window may hold (the substitution stage's rule)
INT32_MAX = 2**31 - 1
OWN_ALL = 2**32 - 1              # own_hi of a whole record
NOTHING = 2**30                  # a min_span no call reaches
ZERO, N, EOS = pystreaks.ZERO, pystreaks.N, pystreaks.EOS


class Planes:
    """the stub pyevents.window_events reads: nmask() and plane(m)"""

    def __init__(self, planes, nmask):
        self._planes, self._nmask = planes, nmask

    def nmask(self):
        return self._nmask

    def plane(self, m):
        return self._planes[m]


def random_plane(rs, length, mean_pass, mean_fail):
    """stretches of ones (mean mean_pass) and of zeros (mean mean_fail), geometric, starting with either"""
    if length == 0:
        return np.zeros(0, np.uint8)
    k = length // 2 + 2
    ones, zeros = rs.geometric(1.0 / mean_pass, k), rs.geometric(1.0 / mean_fail, k)
    runs = np.empty(2 * k, np.int64)
    first = int(rs.randint(2))
    runs[first::2], runs[1 - first::2] = ones, zeros
    bits = np.empty(2 * k, np.uint8)
    bits[first::2], bits[1 - first::2] = 1, 0
    return np.repeat(bits, runs)[:length].copy()


def plane_of(length, stretches, fill=0):
    """a plane of `fill` with the given (first, past-last, bit) stretches written in order"""
    p = np.full(length, fill, np.uint8)
    for a, b, bit in stretches:
        p[max(a, 0):max(min(b, length), 0)] = bit
    return p


def make_record(name, m_lo, m_hi, planes, nmask):
    """planes: {m: bits}; -> the case: planes, N mask, the record's bytes, the streaks as (mlen, start, end, term), motif-major"""
    length = len(nmask)
    nmask = np.asarray(nmask, np.uint8)
    planes = {m: np.asarray(planes[m], np.uint8) for m in range(m_lo, m_hi + 1)}
    assert all(len(p) == length for p in planes.values())
    seq = np.where(nmask == 1, ord("N"), ord("A")).astype(np.uint8).tobytes()
    ev, cnt = pyevents.window_events(Planes(planes, nmask), m_lo, m_hi, ALLOWED)
    streaks = pystreaks.streaks_of(ev, cnt, m_lo)
    return {"name": name, "m_lo": m_lo, "m_hi": m_hi, "L": length, "planes": planes, "nmask": nmask, "seq": seq, "streaks": streaks}


def generate(name, seed, length, m_lo, m_hi, mean_pass, mean_fail, n_blocks=(), same_planes=False):
    """the generator: random stretches per motif (same_planes: the first two motifs share a plane, so that they call at one
    position), N over every [first, past-last) of n_blocks"""
    rs = np.random.RandomState(seed)
    nmask = np.zeros(length, np.uint8)
    for a, b in n_blocks:
        nmask[a:b] = 1
    planes = {m: random_plane(rs, length, mean_pass, mean_fail) for m in range(m_lo, m_hi + 1)}
    if same_planes:
        planes[m_lo + 1] = planes[m_lo]
    return make_record(name, m_lo, m_hi, planes, nmask)


def records_of(streaks):
    """(mlen, start, end, term) tuples -> RUN_DT records in the same order"""
    a = np.array(streaks, dtype="<i4").reshape(-1, 4)
    out = np.zeros(len(a), RUN_DT)
    out["mlen"], out["start"], out["end"], out["term"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return out


def sequential_log(case):
    """the addSeed call log of the literal state machine, cached in the case"""
    if "log" not in case:
        case["log"] = [tuple(int(x) for x in c) for c in
                       pyref.window_calls(case["planes"], case["nmask"], case["m_lo"], case["m_hi"], 8 - ALLOWED)]
    return case["log"]


def in_loop(case):
    """-> (the log's in-loop calls, per call: made at an N or right behind a window that was not evaluated)"""
    if "inloop" not in case:
        L, nmask = case["L"], case["nmask"]
        e = pystreaks.eval_mask(nmask)
        calls = [c for c in sequential_log(case) if c[0] < L]
        case["inloop"] = calls, [bool(nmask[c[0]] or c[0] < 8 or not e[c[0] - 8]) for c in calls]
    return case["inloop"]


def tables(m_lo, m_hi):
    """the min_span tables of the case list: all zero, the two product cut-offs, one that keeps nothing; and two that keep every
    call of every other motif and none of the rest, under which a kept edge call often follows a call that was not kept and ends
    beyond it -- the product cut-offs leave a handful of those per record"""
    ms = range(m_lo, m_hi + 1)
    return {"zero": [0] * len(ms), "subst": [SUBST_SPAN(m) for m in ms], "anchored": [ANCHORED_SPAN(m) for m in ms], "nothing": [NOTHING] * len(ms),
            "first": [NOTHING * (i % 2) for i in range(len(ms))], "second": [NOTHING * (1 - i % 2) for i in range(len(ms))]}


def _rows(calls, shift):
    a = np.array(calls, dtype=np.int64).reshape(-1, 4)
    a[:, (0, 2, 3)] += shift
    return a.astype("<i4")


def expectation(case, table, own_lo=0, own_hi=OWN_ALL, z_lo=0, keep_flush=True, pos_offset=0, full=False):
    """what one call of the hook must return, all from the sequential log: calls and flush ((n, 4) int32: pos, mlen, start, end),
    pend (None or int32), tail_pend, inexact, n_edge, and seen (per kept call the largest end of any earlier owned call)"""
    L, m_lo = case["L"], case["m_lo"]
    calls, edge = in_loop(case)
    idx = [i for i, c in enumerate(calls) if own_lo <= c[0] < own_hi]
    owned, owned_edge = [calls[i] for i in idx], [edge[i] for i in idx]
    span = (lambda m: 0) if full else (lambda m: table[m - m_lo])
    kept, seen, top = [], [], -1
    for c in owned:
        if c[3] - c[2] >= span(c[1]):
            kept.append(c)
            seen.append(top)
        top = max(top, c[3])
    flush = [c for c in sequential_log(case) if c[0] >= L] if keep_flush else []
    pend = None
    if not full:
        again, bounds = pystreaks.compact_bounds(owned, owned_edge, span)
        assert again == kept
        if kept and any(owned_edge):
            pend = np.array([b + pos_offset if b >= 0 else -1 for b in bounds], dtype="<i4")
    return {"calls": _rows(kept, pos_offset), "flush": _rows(flush, pos_offset), "pend": pend,
            "tail_pend": -1 if full or top < 0 else top + pos_offset,
            "inexact": bool(z_lo != 0 and any(c[2] < z_lo + 8 for c in owned + flush)),
            "n_edge": 0 if full else sum(owned_edge),
            "seen": np.array([s + pos_offset if s >= 0 else -1 for s in seen], dtype=np.int64)}


def bounds_hold(calls, pend, seen):
    """The kept calls with their bounds move a merge's cursors as the full call list would: walking the kept calls in order with
    the running maximum of the earlier kept calls' pend and end, and the call's own pend folded in, max(running, end) must be
    max(seen, end), seen being the largest end of ALL earlier owned calls of the full log.  pend None: no bound anywhere."""
    calls = np.asarray(calls)
    ends = (calls["end"] if calls.dtype.names else calls.reshape(-1, 4)[:, 3]).astype(np.int64)      # CALL_DT records or (n, 4) rows
    pend = np.full(len(ends), -1, np.int64) if pend is None else np.asarray(pend, dtype=np.int64)
    seen = np.asarray(seen, dtype=np.int64)
    if not len(ends) == len(pend) == len(seen):
        return False
    if len(ends) == 0:
        return True
    shown = np.maximum.accumulate(np.maximum(pend, ends))                  # by the kept calls up to and including each one
    running = np.maximum(np.concatenate(([-1], shown[:-1])), pend)         # before a call, its own pend folded in
    return bool(np.array_equal(np.maximum(running, ends), np.maximum(seen, ends)))


# ---- dropped groups ------------------------------------------------------------------------------------------------------

def groups_of(case):
    """[(first streak index, past-last index)] of the chains of joined streaks, by the join rule (the streak before was closed by a
    failing window and ends at most 7 before)"""
    st, out, i = case["streaks"], [], 0
    while i < len(st):
        j = i + 1
        while j < len(st) and st[j][0] == st[j - 1][0] and st[j - 1][3] == ZERO and st[j - 1][2] + 7 >= st[j][1]:
            j += 1
        out.append((i, j))
        i = j
    return out


def droppable(case, table):
    """the groups the anchored scan's filter may drop: [(first index, past-last index, end of the last streak)] of the groups whose
    call is in the log's loop part, fails min_span, is made at its end + 8, and which span at most 16 positions"""
    st, m_lo = case["streaks"], case["m_lo"]
    made = set(in_loop(case)[0])
    out = []
    for i, j in groups_of(case):
        if any(s[3] != ZERO for s in st[i:j]):
            continue
        m, start, e = st[i][0], st[i][1], st[j - 1][2]
        if (e + 15, m, start, e + 7) in made and e + 7 - start < table[m - m_lo] and e - start <= 16:
            out.append((i, j, e))
    return out


def without(case, groups):
    """-> (the streaks without the chosen droppable groups, those groups' ends, ascending)"""
    gone = set()
    for i, j, _ in groups:
        gone.update(range(i, j))
    return [s for k, s in enumerate(case["streaks"]) if k not in gone], sorted({e for _, _, e in groups})


# ---- the case list ---------------------------------------------------------------------------------------------------------
# (2, 3): two motifs; (6, 9): four, where the two product tables differ; (30, 32): motif lengths that need six bits of the key

SMALL_LENGTHS = list(range(10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65]
KEY_LENGTHS = [1014, 1015, 1016, 1017, 2038, 2039, 2040, 2041]       # length + 8 straddles 1024 and 2048
PERIOD = 13                      # the periodic plane: 7 ones, a zero, 4 ones, a zero -> 10 passing windows, 3 failing, for ever
PERIODIC_STREAKS = 2200          # per motif


def _periodic(length):
    p = np.ones(length, np.uint8)
    p[7::PERIOD] = 0
    p[12::PERIOD] = 0
    return p


def _tail_case(name, length):
    """random stretches, and at the end of the record: motif 2's last streak closed by a failing window 16 before the end, so that
    its call is made at the last position; motif 3's streak still open"""
    c = generate(name, length, length, 2, 3, 12, 2)
    a, b = c["planes"][2].copy(), c["planes"][3].copy()
    a[length - 60:length - 40] = 0; a[length - 40:length - 10] = 1; a[length - 10:] = 0
    b[length - 60:length - 30] = 0; b[length - 30:] = 1
    return make_record(name, 2, 3, {2: a, 3: b}, c["nmask"])


def _n_every(length, step, seed):
    """single Ns about every `step` bases"""
    rs = np.random.RandomState(seed)
    at = np.cumsum(rs.randint(step // 2, step + step // 2, size=length // step + 1))
    return [(int(x), int(x) + 1) for x in at if x < length]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for length in SMALL_LENGTHS:
        out.append(generate(f"len{length}", 100 + length, length, 2, 3, 12, 2))
    for length in (17, 33, 65):
        out.append(generate(f"len{length}_n", 200 + length, length, 2, 3, 14, 2, n_blocks=[(length // 2, length // 2 + 1)]))
    for length in KEY_LENGTHS:
        out.append(_tail_case(f"key{length}", length))
    # N placement: single Ns at bits 0, 7, 8, 24, 31 of a word; a block over whole words (12 words without an evaluated window);
    # a block longer than a block of the evaluated-window kernel (256 words); a block that runs to the end of the record
    out.append(generate("n_bits", 5, 700, 6, 9, 14, 2, n_blocks=[(64 + 0, 65), (160 + 7, 168), (256 + 8, 265), (352 + 24, 377), (448 + 31, 480), (576, 577)]))
    out.append(generate("n_words", 2, 1200, 2, 3, 12, 2, n_blocks=[(300, 700)]))
    out.append(generate("n_block_9000", 3, 12_000, 2, 3, 12, 2, n_blocks=[(700, 9_900)]))
    out.append(generate("n_to_the_end", 4, 900, 6, 9, 14, 2, n_blocks=[(617, 900)]))
    # gaps of 7 and 8 behind a streak closed by a failing window (two and three zeros in a row), and the smallest gaps behind a
    # streak closed by an N; Ns every 30 bases or so join short streaks to groups that end before and behind them
    g = np.ones(400, np.uint8)
    for at, z in ((40, 2), (80, 3), (120, 2), (122 + 20, 3), (200, 2), (260, 3)):
        g[at:at + z] = 0
    out.append(make_record("gaps_7_8", 2, 3, {2: g, 3: np.roll(g, 5)}, plane_of(400, [(300, 301, 1), (330, 331, 1)])))
    out.append(generate("n_joined", 11, 3000, 2, 3, 9, 1.6, n_blocks=_n_every(3000, 30, 7)))
    # dense: more than 4096 streaks (three blocks of the calls kernel); every streak of a motif in one group, across streak
    # indices 255|256 and 2047|2048; the same with a group that ends exactly at index 2047
    out.append(generate("dense_40k", 1, 40_000, 6, 9, 10, 3, n_blocks=_n_every(40_000, 300, 5)))
    per = _periodic(PERIOD * PERIODIC_STREAKS)
    out.append(make_record("periodic", 2, 3, {2: per, 3: per}, np.zeros(len(per), np.uint8)))
    cut = per.copy()
    cut[PERIOD * 2047 + 7:PERIOD * 2047 + 10] = 0          # the failing stretch behind streak 2047: nine windows, not three
    out.append(make_record("periodic_cut_2047", 2, 3, {2: cut, 3: per}, np.zeros(len(per), np.uint8)))
    # an edge call more than 8192 positions (a block of the word scans) behind the last ordinary call, which is made at 16, the
    # first position there is (zeros at 7 and 8: window 0 passes, window 1 does not)
    far = plane_of(9_200, [(0, 7, 1), (9_000, 9_030, 1)])
    out.append(make_record("look_back", 2, 3, {2: far, 3: np.zeros(9_200, np.uint8)}, plane_of(9_200, [(9_033, 9_034, 1)])))
    # at least 100 edge calls, two motifs of four on one plane; about 70 000 positions with Ns throughout
    out.append(generate("edge_dense", 31, 6_000, 6, 9, 10, 2, n_blocks=_n_every(6_000, 25, 3), same_planes=True))
    out.append(generate("large_70k", 41, 70_000, 30, 32, 11, 2.5, n_blocks=_n_every(70_000, 400, 9) + [(20_000, 29_000)]))
    # dropped groups: random stretches whose short lone streaks the filter may drop, and a record whose last call is one
    out.append(generate("droppable", 51, 12_000, 6, 9, 6, 6))
    d = generate("drop_tail", 52, 2_000, 6, 9, 6, 6)
    planes = {m: p.copy() for m, p in d["planes"].items()}
    for m in planes:
        planes[m][1_900:] = 0
    planes[6][1_950:1_957] = 1                              # seven ones: two passing windows, a call of length 9
    out.append(make_record("drop_tail", 6, 9, planes, d["nmask"]))
    assert len({c["name"] for c in out}) == len(out)
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


def variants(c):
    """the calls of the hook a case is checked with: [dict(table=<name>, full, own_lo, own_hi, z_lo, keep_flush, pos_offset)].
    Whole record under every table and in full mode; then, around calls of the log, own ranges that start or end on a call's
    position, one below and one above, mid-word, empty and one word long, with and without the end-of-sequence calls, a first
    exact position, and the record pushed against INT32_MAX."""
    whole = dict(full=False, own_lo=0, own_hi=OWN_ALL, z_lo=0, keep_flush=True, pos_offset=0)
    out = [dict(whole, table=t) for t in ("zero", "subst", "anchored", "nothing", "first", "second")] + [dict(whole, table="zero", full=True)]
    out.append(dict(whole, table="subst", pos_offset=INT32_MAX - c["L"]))
    out.append(dict(whole, table="zero", keep_flush=False, pos_offset=INT32_MAX - c["L"], z_lo=24))
    calls, edge = in_loop(c)
    if not calls:
        return out
    pick = {0, len(calls) // 2, len(calls) - 1}
    pick.update([i for i, e in enumerate(edge) if e][:2])
    pick.update([i for i, e in enumerate(edge) if e][-1:])
    for k, i in enumerate(sorted(pick)):
        pos, start = calls[i][0], calls[i][2]
        t = ("zero", "anchored", "second", "subst", "first")[k % 5]
        for d in (-1, 0, 1):
            out.append(dict(whole, table=t, own_lo=max(pos + d, 0), keep_flush=d != 0))
            out.append(dict(whole, table=t, own_hi=max(pos + d, 0), keep_flush=d == 0))
        out.append(dict(whole, table=t, own_lo=pos, own_hi=pos))                                              # empty
        out.append(dict(whole, table=t, own_lo=pos // 32 * 32, own_hi=pos // 32 * 32 + 32, keep_flush=False))    # one word
        out.append(dict(whole, table=t, own_lo=max(pos - 45, 0), own_hi=pos + 77))                            # mid-word both ends
        out.append(dict(whole, table="zero", full=True, own_lo=max(pos - 45, 0), own_hi=pos + 1, keep_flush=False))
        out.append(dict(whole, table=t, z_lo=max(start - 7, 1), own_lo=max(pos - 3, 0)))                      # start < z_lo + 8: inexact
        out.append(dict(whole, table=t, z_lo=max(start - 8, 1), own_lo=pos, own_hi=pos + 1, pos_offset=1000))  # start == z_lo + 8: exact
    return out


def drop_variants(c, table_name):
    """the dropped-group runs of a case: [(groups to drop, own_lo, own_hi)]: one group per word offset 16, 17 and 31 of its end
    (its call's bit stays in the word, lands on bit 0 of the next, crosses into it), each alone and all together; own ranges that
    start or end on, one below and one above a dropped call's position; the last droppable group of the record alone"""
    table = tables(c["m_lo"], c["m_hi"])[table_name]
    groups = droppable(c, table)
    out = []
    chosen = []
    for off in (16, 17, 31):
        at = [g for g in groups if g[2] % 32 == off]
        if at:
            chosen.append(at[len(at) // 2])
            out.append(([chosen[-1]], 0, OWN_ALL))
    if chosen:
        out.append((chosen, 0, OWN_ALL))
    for g in [g for g in groups if (g[2] + 15) % 32 not in (0, 31)][:3] + chosen[:1]:
        pos = g[2] + 15
        for d in (-1, 0, 1):
            out.append(([g], pos + d, OWN_ALL))
            out.append(([g], 0, pos + d))
    if groups:
        out.append(([max(groups, key=lambda g: g[2])], 0, OWN_ALL))
        out.append((groups, 0, OWN_ALL))
    return out
