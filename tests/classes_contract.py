"""The contract of the rows by canonical motif class (include/ribbit_hip.h) in plain Python: the class of a motif is the minimum
over the 2k strings that are its rotations and the rotations of its reverse complement, the strand is membership among its own
rotations; the groups are a dict, their order a sorted() by (length, class).  Slow and obviously right: what the host twin
(ribbit_host_record_classes) and the kernels (classes.hip) are compared with."""
import numpy as np

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
# where the code takes another path: the key holds 27 bases, a register 32, a wave 64 lanes; -M ends at 990, the contract at 1023
MOTIF_LENGTHS = (1, 2, 26, 27, 28, 31, 32, 33, 63, 64, 65, 127, 128, 129, 500, 990, 1023)


def reverse_complement(u):
    return "".join(COMPLEMENT[c] for c in reversed(u))


def rotations(u):
    return [u[i:] + u[:i] for i in range(len(u))]


def motif_class(u):
    """-> (class, strand)"""
    assert u and set(u) <= set("ACGT") and len(u) <= 1023
    own = rotations(u)
    cls = min(own + rotations(reverse_complement(u)))      # (str order is byte order, and A < C < G < T in ASCII)
    return cls, "+" if cls in own else "-"


def clipped_widths(length, intervals):
    return [max(0, min(int(e), length) - max(int(s), 0)) for s, e in intervals]


def record_classes(length, intervals, motifs):
    """-> (the class of every row, the strand of every row, the groups in class order as (class, length, rows, bases, first_row,
    longest_row))"""
    assert len(intervals) == len(motifs)
    classes, strands, members = [], [], {}
    for i, u in enumerate(motifs):
        cls, strand = motif_class(u)
        classes.append(cls)
        strands.append(strand)
        members.setdefault(cls, []).append(i)
    width = clipped_widths(length, intervals)
    groups = []
    for cls in sorted(members, key=lambda c: (len(c), c)):
        rows = members[cls]
        longest = min(rows, key=lambda i: (-width[i], i))
        groups.append((cls, len(cls), len(rows), sum(width[i] for i in rows), rows[0], longest))
    return classes, strands, groups


def check_properties(length, intervals, motifs, classes, strands, groups):
    """what follows from the contract, checked on a result however it was made"""
    n = len(motifs)
    assert len(classes) == len(strands) == n
    for u, cls, strand in zip(motifs, classes, strands):
        assert len(cls) == len(u)
        assert motif_class(cls) == (cls, "+")                              # the class of the class is the class, on '+'
        assert motif_class(reverse_complement(u))[0] == cls               # the class of the reverse complement is the class
        assert strand in "+-" and (strand == "+") == (cls in rotations(u))
    assert sum(g[2] for g in groups) == n
    assert sum(g[3] for g in groups) == sum(clipped_widths(length, intervals))
    keys = [(g[1], g[0]) for g in groups]
    assert all(a < b for a, b in zip(keys, keys[1:]))                      # the groups strictly ascend
    width = clipped_widths(length, intervals)
    for cls, k, rows, bases, first, longest in groups:
        assert k == len(cls) and rows >= 1 and classes[first] == cls and classes[longest] == cls
        assert first == classes.index(cls) and first <= longest
        assert all(width[i] < width[longest] or (width[i] == width[longest] and i >= longest) for i in range(n) if classes[i] == cls)


def random_motif(rs, k, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rs.randint(0, len(alphabet), k))


def periodic(unit, k):
    return (unit * (k // len(unit) + 1))[:k]


def key_twins(rs, k):
    """motifs of k >= 28 bases that are their own class (eight A in front, then C and G only: no other rotation, and none of the
    reverse complement, which has no A at all, starts as low), equal in their first 27 bases: one, the same with base 28 changed,
    the same with the last base changed, and the first again"""
    body = "A" * 8 + random_motif(rs, k - 8, "CG")
    swap = {"C": "G", "G": "C"}
    return [body, body[:27] + swap[body[27]] + body[28:], body[:-1] + swap[body[-1]], body]


def edge_case_sets(length):
    """[(intervals, motifs)]: the contract's corners on a record of `length` bases"""
    rs = np.random.RandomState(length + 11)
    sets = []
    # motifs that are their own reverse complement, homopolymers, periodic motifs in which every rotation ties
    own = ["AT", "TA", "ACGT", "CGTA", "AATT", "TTAA", "A", "T", "C", "G", "ACAC", "CACA", "GTGT", "ACGACG", "CGTCGT", periodic("ACG", 990), periodic("TCG", 990),
           periodic("AC", 64), periodic("GT", 33)]
    sets.append(([(3 * i, 3 * i + 10 + i) for i in range(len(own))], own))
    # CA, AC, TG, GT and the rotations of GATA and of TATC are one class each
    one = ["CA", "AC", "TG", "GT", "GATA", "ATAG", "TAGA", "AGAT", "TATC", "ATCT", "TCTA", "CTAT"]
    sets.append(([(5, 9)] * len(one), one))
    # long motifs equal in their first 27 bases that differ at base 28, and at the last base: the key alone cannot part these
    for k in (28, 33, 64, 500, 1023):
        twins = key_twins(rs, k)
        twins += [reverse_complement(u[5:] + u[:5]) for u in twins]
        sets.append(([(i, i + 50) for i in range(len(twins))], twins))
    # longest_row ties go to the lowest index; empty and out-of-range rows count as rows of 0 bases
    sets.append(([(10, 20), (30, 40), (5, 15), (40, 30), (length + 5, length + 50), (-30, -2), (0, 10)], ["AC", "CA", "GT", "AC", "AC", "TG", "AAC"]))
    sets.append(([(9, 5), (7, 7), (length, length + 3)], ["AG", "CT", "GA"]))
    sets.append(([(-5, length + 5)], ["ACGTT"]))
    sets.append(([], []))
    return sets


def random_record(rs, t):
    """(length, intervals, motifs): a few classes with many rows each, some rows empty or out of range, motif lengths of every path"""
    length = int(rs.randint(0, 5000))
    n = int(rs.randint(1, 120))
    lengths = [int(rs.choice(MOTIF_LENGTHS[:8])) for _ in range(4)] + ([int(rs.choice(MOTIF_LENGTHS))] if t % 3 == 0 else [])
    units = [random_motif(rs, k, "ACGT" if t % 2 else "AC") for k in lengths]
    motifs = []
    for _ in range(n):
        u = units[rs.randint(0, len(units))]
        r = int(rs.randint(0, len(u)))
        u = u[r:] + u[:r]
        motifs.append(reverse_complement(u) if rs.randint(0, 2) else u)
    starts = rs.randint(-20, length + 20, n)
    return length, np.stack([starts, starts + rs.randint(-5, 300, n)], 1), motifs
