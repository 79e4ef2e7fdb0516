"""The plain statement of the panel contract (include/ribbit_hip.h): which primer pairs may not share a tube, their degrees, the
Welsh-Powell order and the first-fit pools.  Loops over pairs and letters that read like the contract; the duplex is
primer_pairs_contract's, so `any` and `end` have one definition.  The pinned values the header quotes are at the end, with the text
formatter of ribbit_bed_panel_text."""
import functools

import primer_pairs_contract as pp
import primer_products_contract as prc

DEFAULTS = dict(max_cross_any=6, max_cross_end=4, size_gap=30, max_cross_product=4000, pool_size=8)
RANGES = dict(max_cross_any=(0, 32), max_cross_end=(0, 32), size_gap=(0, 100000), max_cross_product=(0, 1 << 30), pool_size=(1, 65536))
MAX_PAIRS, MAX_DEBUG_PAIRS = 65536, 8192
FIELDS = ("pool", "conflicts", "dimer", "size", "near", "reserved0", "reserved1", "reserved2")
NOT_POOLED = (-1, 0, 0, 0, 0, 0, 0, 0)
NO_PAIR = (-1, 0, 0, 0, 0, 0) * 2 + (0,) * 20


def params(**fields):
    assert set(fields) <= set(DEFAULTS)
    return dict(DEFAULTS, **fields)


def pair(a: str, b: str, left_start: int, right_start: int):
    """a hand-made row of 32 values: the left primer a at left_start and the right primer b (as ordered, 5' to 3') whose forward-strand
    bases start at right_start, and the product they span; all else 0"""
    row = list(prc.pair_tuple(a, b, left_start, right_start))
    row[14] = right_start + len(b) - left_start
    return tuple(row)


def has_pair(row) -> bool:
    return row[0] >= 0


def extras(pairs, extra):
    """(group, size_lo, size_hi) of every pair; None: (-1, product, product)"""
    if extra is None:
        return [(-1, r[14], r[14]) for r in pairs]
    out = [tuple(int(v) for v in e) for e in extra]
    assert len(out) == len(pairs)
    return out


@functools.lru_cache(maxsize=None)
def duplex(x: str, y: str):
    return pp.duplex(x, y)


def rules(ri, rj, ei, ej, prm, duplex_of=duplex):
    """-> (dimer, size, near) of two different rows that both have a pair"""
    dimer = False
    for x in prc.oligos_of(ri):
        for y in prc.oligos_of(rj):
            any_, end = duplex_of(x, y)
            dimer = dimer or any_ > prm["max_cross_any"] or end > prm["max_cross_end"]
    gap = prm["size_gap"]
    size = gap > 0 and ei[1] - ej[2] < gap and ej[1] - ei[2] < gap
    span_i, span_j = (ri[0], ri[6] + ri[7]), (rj[0], rj[6] + rj[7])
    hull = max(span_i[1], span_j[1]) - min(span_i[0], span_j[0])
    near = prm["max_cross_product"] > 0 and ei[0] == ej[0] and ei[0] >= 0 and hull <= prm["max_cross_product"]
    return dimer, size, near


def conflict_rules(pairs, extra=None, prm=None, duplex_of=duplex):
    """-> n x n (dimer, size, near), all False on the diagonal and wherever a row has no pair"""
    prm, ex, n = prm or DEFAULTS, extras(pairs, extra), len(pairs)
    out = [[(False, False, False)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if has_pair(pairs[i]) and has_pair(pairs[j]):
                out[i][j] = out[j][i] = rules(pairs[i], pairs[j], ex[i], ex[j], prm, duplex_of)
    return out


def conflict_matrix(pairs, extra=None, prm=None, duplex_of=duplex):
    """-> n x n booleans"""
    return [[any(r) for r in row] for row in conflict_rules(pairs, extra, prm, duplex_of)]


def matrix_words(matrix):
    """the booleans as ribbit_hip_debug_panel_conflicts lays them out: n rows of (n + 63) // 64 words, bit j % 64 of word j // 64"""
    n = len(matrix)
    return [[sum(1 << (j - 64 * w) for j in range(64 * w, min(n, 64 * w + 64)) if row[j]) for w in range((n + 63) // 64)] for row in matrix]


def pools_of(pairs, rule_matrix, pool_size):
    """degrees, the order and the first fit from the three rules of every (i, j) -> (one tuple of FIELDS per pair, the pools)"""
    n = len(pairs)
    counts = [[sum(1 for r in row if r[k]) for k in range(3)] + [sum(1 for r in row if any(r))] for row in rule_matrix]
    order = sorted((i for i in range(n) if has_pair(pairs[i])), key=lambda i: (-counts[i][3], i))
    members, pool_of = [], {}
    for i in order:
        for p, inside in enumerate(members):
            if len(inside) < pool_size and not any(any(rule_matrix[i][j]) for j in inside):
                break
        else:
            p = len(members)
            members.append([])
        members[p].append(i)
        pool_of[i] = p
    rows = [(pool_of[i], counts[i][3], counts[i][0], counts[i][1], counts[i][2], 0, 0, 0) if i in pool_of else NOT_POOLED for i in range(n)]
    return rows, len(members)


def panel_pools(pairs, extra=None, prm=None, duplex_of=duplex):
    prm = prm or DEFAULTS
    return pools_of(pairs, conflict_rules(pairs, extra, prm, duplex_of), prm["pool_size"])


def as_tuples(arr):
    return [tuple(int(v) for v in r) for r in arr.tolist()]


# ---- the text
def panel_lines(marker_text: str, rows, products) -> str:
    """the members' marker lines with the five columns, by (pool, designed product, input order); products: the pairs' designed
    product sizes (column 20 of a marker line)"""
    lines = marker_text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) == len(rows) == len(products)
    members = sorted((r[0], products[i], i) for i, r in enumerate(rows) if r[0] >= 0)
    return "".join(lines[i] + "".join("\t" + str(v) for v in rows[i][:5]) + "\n" for _, _, i in members)


# ---- the pinned values
L, RB = "GATTACAGATTACAGGCT", pp.reverse_complement("CCTGAAGTCTCGGATCAA")      # the pair of the in-silico PCR contract
DIMER_A, DIMER_B = "GATTACAGATTACAGGC", "TTTGCCTGTAATC"                         # duplex (10, 10)
# eight oligos of which no two, nor one with itself or with DIMER_A or DIMER_B, exceed (6, 4)
QUIET = ("TTCAGGACCTAACCTGAG", "TAGCCAAGTTCAACGGCAG", "TGCAACCTAGGGAGAATGTG", "ACATACGCTCTTACTGCGGTC",
         "CGGAGCATAAATCCCACC", "GAACTAAGTTTGTCGAACC", "GGTAAACGAACCGTTGCG", "AATTTGAAGCAGTGGCCGGG")


def quiet_pair(k: int, left_start: int, product: int):
    """pair k of four made of QUIET: its oligos bind nothing in the set"""
    a, b = QUIET[2 * k], QUIET[2 * k + 1]
    return pair(a, b, left_start, left_start + product - len(b))


def pinned_cases():
    """name -> (pairs, extra, params' fields, the pools of the pairs, the number of pools, (conflicts, dimer, size, near) of every pair)"""
    q = [quiet_pair(k, 1000 * k, 100 + 50 * k) for k in range(4)]
    near_a, near_b = quiet_pair(0, 0, 100), quiet_pair(1, 3850, 150)      # hull 4000
    far_b = quiet_pair(1, 3851, 150)                                     # hull 4001
    star = [quiet_pair(k, 0, 100 + 100 * k) for k in range(3)] + [quiet_pair(3, 0, 200)]
    dimers = [pair(DIMER_A, QUIET[0], 0, 100), pair(QUIET[2], DIMER_B, 0, 200)]
    return {
        "no conflict": (q[:2], None, {}, [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "dimer": (dimers, None, {}, [0, 1], 2, [(1, 1, 0, 0)] * 2),
        "size at gap 30": ([quiet_pair(0, 0, 100), quiet_pair(1, 0, 129)], None, {}, [0, 1], 2, [(1, 0, 1, 0)] * 2),
        "size at gap 30, 30 apart": ([quiet_pair(0, 0, 100), quiet_pair(1, 0, 130)], None, {}, [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "size at gap 0": ([quiet_pair(0, 0, 100), quiet_pair(1, 0, 129)], None, dict(size_gap=0), [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "near at hull 4000": ([near_a, near_b], [(5, 100, 100), (5, 150, 150)], {}, [0, 1], 2, [(1, 0, 0, 1)] * 2),
        "near at hull 4001": ([near_a, far_b], [(5, 100, 100), (5, 150, 150)], {}, [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "near in different groups": ([near_a, near_b], [(5, 100, 100), (6, 150, 150)], {}, [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "near with the groups unknown": ([near_a, near_b], [(-1, 100, 100), (-1, 150, 150)], {}, [0, 0], 1, [(0, 0, 0, 0)] * 2),
        "pool_size 1": (q[:3], None, dict(pool_size=1), [0, 1, 2], 3, [(0, 0, 0, 0)] * 3),
        "star": (star, [(-1, 100, 100), (-1, 200, 200), (-1, 300, 300), (-1, 90, 310)], {}, [1, 1, 1, 0], 2, [(1, 0, 1, 0)] * 3 + [(3, 0, 3, 0)]),
        "a row without a pair": ([q[0], NO_PAIR, q[1]], None, {}, [0, -1, 0], 1, [(0, 0, 0, 0)] * 3),
        "the limits at 32": (dimers, None, dict(max_cross_any=32, max_cross_end=32), [0, 0], 1, [(0, 0, 0, 0)] * 2),
    }


def pinned_rows(case):
    pairs, _, _, pools, _, counts = case
    return [(p,) + c + (0, 0, 0) if p >= 0 else NOT_POOLED for p, c in zip(pools, counts)]
