"""The contract of the nearest target of every query stated in plain Python (tests/test_nearest.py, tests/test_nearest_gpu.py;
include/ribbit_hip.h has the words): a loop over the queries with a loop over the targets inside, no sort beyond min and max
with keys.  The properties that follow from it, the plain formatter of the two texts, and the interval sets on which the tests
compare an implementation with it."""
import numpy as np

import overlap_contract

FIELDS = ("kind", "hit", "left", "left_dist", "right", "right_dist")
APART, OVER, INSIDE = 0, 1, 2
NOTHING = (APART, -1, -1, -1, -1, -1)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def clipped(length, intervals):
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    return [(max(int(s), 0), min(int(e), length)) for s, e in iv]


def record_nearest(length, queries, targets):
    """-> one (kind, hit, left, left_dist, right, right_dist) per query"""
    live = [(s, e, j) for j, (s, e) in enumerate(clipped(length, targets)) if s < e]
    order_a = lambda t: (t[0], t[1], t[2])
    order_b = lambda t: (t[1], t[0], t[2])
    out = []
    for s, e in clipped(length, queries):
        if s >= e:
            out.append(NOTHING)
            continue
        kind, hit = APART, -1
        holding = [t for t in live if t[0] <= s and t[1] >= e]
        meeting = [t for t in live if t[0] < e and t[1] > s]
        if holding:
            furthest = max(t[1] for t in holding)
            kind, hit = INSIDE, min((t for t in holding if t[1] == furthest), key=order_a)[2]
        elif meeting:
            kind, hit = OVER, min(meeting, key=order_a)[2]
        left, left_dist, right, right_dist = -1, -1, -1, -1
        before = [t for t in live if t[1] <= s]
        behind = [t for t in live if t[0] >= e]
        if before:
            t = max(before, key=order_b)
            left, left_dist = t[2], s - t[1]
        if behind:
            t = min(behind, key=order_a)
            right, right_dist = t[2], t[0] - e
        out.append((kind, hit, left, left_dist, right, right_dist))
    return out


def record_nearest_without_loops(length, queries, targets):
    """record_nearest for sets too large for its double loop, with numpy alone: the targets in both orders by lexsort, the running
    maximum of the ends along order A, and every field by searchsorted -> an (n, 6) int64 array.  (The tests hold it against
    record_nearest on the small sets before they rely on it.)"""
    def clip(iv):
        iv = np.asarray(iv, np.int64).reshape(-1, 2)
        return np.maximum(iv[:, 0], 0), np.minimum(iv[:, 1], length)
    ts, te = clip(targets)
    j = np.flatnonzero(ts < te)
    ts, te = ts[j], te[j]
    m = len(j)
    a, b = np.lexsort((j, te, ts)), np.lexsort((j, ts, te))
    a_s, a_e, a_j, b_e, b_j = ts[a], te[a], j[a], te[b], j[b]
    reach = np.maximum.accumulate(a_e) if m else a_e
    rises = np.concatenate([[True], a_e[1:] > reach[:-1]]) if m else np.zeros(0, bool)
    reach_at = np.maximum.accumulate(np.where(rises, np.arange(m), 0)) if m else np.zeros(0, np.int64)
    pad = lambda x: np.concatenate([x, [0]])              # (so that an index that is not used can still be looked up)
    qs, qe = clip(queries)
    has = qs < qe
    pa, pe, pb = np.searchsorted(a_s, qs, "right"), np.searchsorted(a_s, qe, "left"), np.searchsorted(b_e, qs, "right")
    po = np.searchsorted(reach, qs, "right")
    inside = has & (pa > 0) & (pad(reach)[pa - 1] >= qe)
    over = has & ~inside & (po < pe)
    left, right = has & (pb > 0), has & (pe < m)
    out = np.full((len(qs), 6), -1, np.int64)
    out[:, 0] = np.where(inside, INSIDE, np.where(over, OVER, APART))
    out[:, 1] = np.where(inside, pad(a_j)[pad(reach_at)[pa - 1]], np.where(over, pad(a_j)[np.minimum(po, m)], -1))
    out[:, 2] = np.where(left, pad(b_j)[pb - 1], -1)
    out[:, 3] = np.where(left, qs - pad(b_e)[pb - 1], -1)
    out[:, 4] = np.where(right, pad(a_j)[np.minimum(pe, m)], -1)
    out[:, 5] = np.where(right, pad(a_s)[np.minimum(pe, m)] - qe, -1)
    return out


def as_array(nearest):
    """a NEAREST_DT array as record_nearest_without_loops returns its result"""
    return np.stack([np.asarray(nearest[f], np.int64) for f in FIELDS], 1) if len(nearest) else np.zeros((0, 6), np.int64)


def as_tuples(nearest):
    """a NEAREST_DT array as the list record_nearest returns"""
    return [tuple(int(r[f]) for f in FIELDS) for r in nearest]


def check_properties(length, queries, targets, nearest):
    """what follows from the contract, checked on a result in the form of record_nearest's"""
    q, t = clipped(length, queries), clipped(length, targets)
    live = [(s, e) for s, e in t if s < e]
    counts, _ = overlap_contract.record_overlap(length, queries, targets)
    assert len(nearest) == len(q)
    for i, ((s, e), (kind, hit, left, left_dist, right, right_dist)) in enumerate(zip(q, nearest)):
        if s >= e:
            assert (kind, hit, left, left_dist, right, right_dist) == NOTHING
            continue
        # kind and the overlap count
        assert (kind > 0) == (counts[i][0] > 0), i
        assert (hit >= 0) == (kind > 0)
        # containment: every base of the query inside one target
        assert (kind == INSIDE) == any(ts <= s and te >= e for ts, te in live), i
        if kind == INSIDE:
            assert t[hit][0] <= s and t[hit][1] >= e
        if kind == OVER:
            assert t[hit][0] < t[hit][1] and t[hit][0] < e and t[hit][1] > s
        # neighbours: they do not overlap the query, and nothing non-empty lies between them and it
        if left >= 0:
            ls, le = t[left]
            assert ls < le <= s and left_dist == s - le
            assert not any(le < te <= s for _, te in live), i
        else:
            assert left_dist == -1 and not any(te <= s for _, te in live), i
        if right >= 0:
            rs, re = t[right]
            assert e <= rs < re and right_dist == rs - e
            assert not any(e <= ts < rs for ts, _ in live), i
        else:
            assert right_dist == -1 and not any(ts >= e for ts, _ in live), i


def check_symmetry(length, queries, targets, forward, backward):
    """forward: the queries against the targets, backward: the targets against the queries.  A query that is apart and has target
    j to its right at distance d: j as a query has a left neighbour at a distance of d at most."""
    q = clipped(length, queries)
    for (s, e), (kind, _, _, _, right, right_dist) in zip(q, forward):
        if s < e and kind == APART and right >= 0:
            assert backward[right][2] >= 0 and 0 <= backward[right][3] <= right_dist


# ---- the two texts
def _label(labels, j):
    if j < 0:
        return "."
    text = labels[j] if isinstance(labels[j], str) else labels[j].decode()
    return text if text else "."


def eight_columns(near, targets, labels):
    kind, hit, left, left_dist, right, right_dist = near
    cols = [("in" if kind == INSIDE else "over" if kind == OVER else "."), _label(labels, hit)]
    cols += [str(int(targets[hit][0])), str(int(targets[hit][1]))] if hit >= 0 else [".", "."]
    cols += [_label(labels, left), str(left_dist) if left >= 0 else "."]
    cols += [_label(labels, right), str(right_dist) if right >= 0 else "."]
    return cols


def nearest_lines(bed, nearest, targets, labels):
    """the --nearest-bed lines of one record: every line of its BED text with the eight columns behind it"""
    rows = bed.splitlines()
    assert len(rows) == len(nearest)
    return "".join("\t".join([line] + eight_columns(near, targets, labels)) + "\n" for line, near in zip(rows, nearest))


def other_lines(name, targets, labels, nearest, rows, motifs):
    """the --nearest-other-bed lines of one record: one per interval of the other file, with the rows as the targets"""
    assert len(targets) == len(nearest) == len(labels)
    return "".join("\t".join([name, str(int(s)), str(int(e)), _label(labels, j)] + eight_columns(near, rows, motifs)) + "\n"
                   for j, ((s, e), near) in enumerate(zip(targets, nearest)))


# ---- the sets
def edge_case_sets(length):
    """[(what, queries, targets)]: the shapes of the issue on a record of `length` bases, small enough for the double loop"""
    L = length
    mid = L // 2
    return [
        ("nothing", [], []),
        ("no queries", [], [(0, L), (3, 9)]),
        ("no targets", [(0, L), (3, 9), (5, 5)], []),
        ("one target", [(0, 1), (mid, mid + 4), (L - 1, L), (0, L), (2, 3)], [(mid, mid + 4)]),
        ("two targets", [(0, 1), (mid, mid + 4), (L - 1, L), (0, L), (mid + 1, mid + 2), (mid + 4, mid + 9)], [(mid, mid + 4), (mid + 2, mid + 30)]),
        ("an empty and a real target", [(0, L), (1, 2), (mid, mid + 1)], [(7, 7), (mid, mid + 3)]),
        ("only empty targets", [(0, L), (1, 2)], [(7, 7), (9, 2), (L, L + 4), (-5, 0)]),
        ("past both ends", [(-100, -1), (L, L + 50), (-7, 3), (L - 1, L + 1000), (-3, L + 3), (1, L - 1)], [(-5, 2), (L - 2, L + 3), (-3, L + 3), (L, L + 9), (-9, 0)]),
        ("reversed and negative", [(50, 10), (20, 20), (90, -5), (10, 50), (-9, 0), (-20, -10)], [(30, 30), (40, 5), (12, 14), (-4, -8), (-8, -4), (45, 60)]),
        ("the int32 limits", [(I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN, 1), (L - 1, I32_MAX), (I32_MAX, I32_MAX), (I32_MIN, I32_MIN), (3, 4)],
         [(I32_MIN, I32_MAX), (I32_MIN, 2), (L - 2, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN, I32_MIN + 1), (I32_MAX - 1, I32_MAX)]),
        ("duplicates", [(20, 30), (20, 30), (25, 28), (100, 130), (0, 5), (40, 90)], [(25, 28)] * 4 + [(100, 130)] * 3 + [(0, 0)] * 2 + [(20, 30)] * 2),
        ("nested", [(12, 14), (10, 40), (5, 45), (21, 22), (30, 41), (0, 3), (50, 60)], [(10, 40), (11, 39), (12, 38), (10, 20), (10, 40), (20, 41), (0, 50), (1, 50)]),
        ("abutting", [(10, 20), (20, 40), (40, 50), (64, 96), (0, 10), (50, 64)], [(20, 40), (0, 10), (50, 64), (96, 97), (32, 64), (10, 20)]),
        ("a query equal to a target", [(3, 9), (40, 50), (70, 80), (0, L)], [(40, 50), (3, 9), (0, L), (70, 80), (70, 80)]),
        ("a wave and one", [(k * 3, k * 3 + 5 + k % 7) for k in range(65)], [(k * 5 + 1, k * 5 + 2 + k % 4) for k in range(65)]),
    ]


def random_sets(length, rs, n, n_targets, longest, reach=3):
    """seeded random queries and targets, some reaching `reach` bases outside the record, some empty or reversed"""
    def one(m):
        starts = rs.randint(-reach, length + reach + 1, m)
        return np.stack([starts, starts + rs.randint(-2, longest, m)], 1).astype(np.int64) if m else np.zeros((0, 2), np.int64)
    return one(n), one(n_targets)
