"""The contract of the best non-overlapping rows stated in plain Python (tests/test_best.py, tests/test_best_gpu.py;
include/ribbit_hip.h has the words): the clipped rows ordered by (e', s', index), one forward sweep, one backward sweep with the
strict comparison.  And a brute force over all subsets for small sets, and the interval sets on which the tests compare an
implementation with the contract."""
import bisect
import itertools

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def clipped(length, intervals):
    """[(s', e')] per row, clipped as the mask clips them"""
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    return [(max(int(s), 0), min(int(e), length)) for s, e in iv]


def record_best(length, intervals):
    """-> (indices of the selected rows by ascending start, the bases they cover)"""
    order = sorted((e, s, i) for i, (s, e) in enumerate(clipped(length, intervals)) if s < e)
    ends = [e for e, _, _ in order]
    r = len(order)
    dp, p = [0] * (r + 1), [0] * (r + 1)
    for k in range(1, r + 1):
        e, s, _ = order[k - 1]
        p[k] = bisect.bisect_right(ends, s)
        dp[k] = max(dp[k - 1], e - s + dp[p[k]])
    chosen, k = [], r
    while k > 0:
        e, s, i = order[k - 1]
        if e - s + dp[p[k]] > dp[k - 1]:
            chosen.append(i)
            k = p[k]
        else:
            k -= 1
    return chosen[::-1], dp[r]


def brute_force_bases(length, intervals):
    """the most bases any set of pairwise non-overlapping rows covers, over all subsets (a dozen rows at most)"""
    rows = [(s, e) for s, e in clipped(length, intervals) if s < e]
    assert len(rows) <= 12
    best = 0
    for mask in range(1 << len(rows)):
        picked = sorted(rows[i] for i in range(len(rows)) if mask >> i & 1)
        if all(a[1] <= b[0] for a, b in zip(picked, picked[1:])):
            best = max(best, sum(e - s for s, e in picked))
    return best


def edge_case_sets(length):
    """the sets of tests/test_loci_gpu.py's edge cases: empty, reversed, out of range, the int32 limits, duplicates, nested, abutting"""
    return [[], [(0, 1)], [(0, length)], [(3, 9), (5, 20)], [(-5, 4), (length - 2, length + 50)], [(I32_MIN, I32_MAX)],
            [(50, 10), (20, 20), (90, -5)], [(50, 10), (10, 50), (20, 20), (200, 220), (90, -5)],
            [(20, 30)] * 5 + [(100, 130)] * 3, [(10, 200), (20, 190), (30, 180), (40, 170), (50, 60), (10, 200)],
            [(10, 20), (20, 30), (30, 31), (40, 50)], [(100, 130), (90, 120), (110, 140), (95, 100)],
            [(length - 1, length)], [(length, length + 1)], [(-1, 0)]]


def random_record(rs, t):
    """(length, rows) as tests/test_loci_gpu.py::test_random_records draws them: length 1000..40000, 0..400 rows, some out of range,
    empty or reversed, every other set with rows up to 3000 long"""
    length = int(rs.randint(1000, 40_000))
    n = int(rs.randint(0, 400))
    starts = rs.randint(-100, length + 100, n)
    return length, np.stack([starts, starts + rs.randint(-20, 3000 if t % 2 else 60, n)], 1)


def check_properties(length, intervals, chosen, bases):
    """what follows from the contract, checked on a selection: the rows are non-empty, ascending by start and pairwise non-overlapping,
    they cover `bases` bases, and of identical rows the lowest index is the one chosen"""
    rows = clipped(length, intervals)
    picked = [rows[i] for i in chosen]
    assert all(s < e for s, e in picked)
    assert all(a[1] <= b[0] for a, b in zip(picked, picked[1:]))
    assert sum(e - s for s, e in picked) == bases
    first = {}
    for i, row in enumerate(rows):
        first.setdefault(row, i)
    assert all(first[rows[i]] == i for i in chosen)
