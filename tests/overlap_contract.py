"""The contract of the rows' overlap with a second set of intervals stated with numpy (tests/test_overlap.py,
tests/test_overlap_gpu.py; include/ribbit_hip.h has the words): a per-base boolean array for each of the two sets, a double
loop over the clipped intervals for `others`, and sums of the arrays for everything else.  And the interval sets on which the
tests compare an implementation with it."""
import numpy as np

TOTALS = ("rows", "rows_hit", "other", "other_hit", "rows_bases", "other_bases", "both_bases")
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _clipped(length, intervals):
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    return [(max(int(s), 0), min(int(e), length)) for s, e in iv]


def _union(length, clipped):
    held = np.zeros(length, bool)
    for s, e in clipped:
        if s < e:
            held[s:e] = True
    return held


def record_overlap(length, rows, other):
    """-> (list of [others, bases] per row, dict of the totals)"""
    a, b = _clipped(length, rows), _clipped(length, other)
    u_rows, u_other = _union(length, a), _union(length, b)
    per_row = []
    for s, e in a:
        if s >= e:
            per_row.append([0, 0])
            continue
        others = 0
        for so, eo in b:
            if so < eo and so < e and eo > s:
                others += 1
        per_row.append([others, int(u_other[s:e].sum())])
    totals = {
        "rows": sum(s < e for s, e in a),
        "rows_hit": sum(s < e and bases > 0 for (s, e), (_, bases) in zip(a, per_row)),
        "other": sum(s < e for s, e in b),
        "other_hit": sum(s < e and bool(u_rows[s:e].any()) for s, e in b),
        "rows_bases": int(u_rows.sum()),
        "other_bases": int(u_other.sum()),
        "both_bases": int((u_rows & u_other).sum()),
    }
    return per_row, totals


def overlap_lines(bed, per_row):
    """the --overlap-bed lines of one record in plain Python: every line of its BED text with the row's two values behind it"""
    rows = bed.splitlines()
    assert len(rows) == len(per_row)
    return "".join(f"{line}\t{others}\t{bases}\n" for line, (others, bases) in zip(rows, per_row))


def summary_line(name, length, totals):
    return "\t".join([name, str(length)] + [str(totals[k]) for k in TOTALS]) + "\n"


def edge_positions(length):
    """the positions at which the kernels change what they do, each with one to either side: the record's ends, the bitmap's word
    edge (32), a lane's block of 8 words (256) and a wave's 64 blocks (16384)"""
    marks = {0, length}
    for unit in (32, 256, 16384):
        marks.update({unit, (length // unit) * unit, max(length // unit - 1, 0) * unit})
    return sorted({p + d for p in marks for d in (-1, 0, 1) if -1 <= p + d <= length + 1})


def edge_case_sets(length):
    """[(what, rows, other)]: the shapes of the issue on a record of `length` bases, small enough for the double loop"""
    L = length
    edges = edge_positions(L)
    # every edge as a start and as an end: from each to the next, and 40 bases to either side of each
    on_edges = list(zip(edges, edges[1:])) + [(p, p + 40) for p in edges] + [(p - 40, p) for p in edges]
    mid = L // 2
    cases = [
        ("nothing", [], []),
        ("no rows", [], [(0, L), (3, 9)]),
        ("no other", [(0, L), (3, 9)], []),
        ("one row", [(mid, mid + 7)], [(mid + 3, mid + 4), (mid - 2, mid + 1)]),
        ("on the edges", on_edges, on_edges[::-2]),
        ("edges against the whole record", on_edges, [(0, L)]),
        ("the whole record against edges", [(0, L)], on_edges),
        ("spanning blocks", [(5, L - 5), (250, 530), (31, 16400)], [(0, 257), (255, 16385), (L - 300, L)]),
        ("out of range", [(-100, -1), (L, L + 50), (-7, 3), (L - 1, L + 1000), (I32_MIN, I32_MAX)], [(-5, 2), (L - 2, I32_MAX), (I32_MIN, 1), (L, I32_MAX)]),
        ("empty and reversed", [(50, 10), (20, 20), (90, -5), (10, 50), (L + 5, L + 9), (-9, 0)], [(30, 30), (40, 5), (12, 14), (I32_MAX, I32_MIN), (L, L)]),
        ("duplicates", [(20, 30)] * 3 + [(100, 130)] * 2, [(25, 28)] * 4 + [(100, 130)] * 3 + [(0, 0)] * 2),
        ("abutting", [(10, 20), (40, 50), (64, 96)], [(20, 40), (0, 10), (50, 64), (96, 97), (32, 64)]),
        ("one word", [(3, 9), (40, 50), (70, 80)], [(10, 20), (45, 47), (60, 75), (79, 81)]),
        ("a wave and one", [(k * 3, k * 3 + 5 + k % 7) for k in range(65)], [(k * 5 + 1, k * 5 + 2 + k % 4) for k in range(65)]),
    ]
    return cases


def random_sets(length, rs, n, n_other, longest):
    """seeded random rows and OTHER intervals, some out of range, some empty or reversed"""
    def one(m):
        starts = rs.randint(-50, length + 50, m)
        return np.stack([starts, starts + rs.randint(-5, longest, m)], 1).astype(np.int64) if m else np.zeros((0, 2), np.int64)
    return one(n), one(n_other)
