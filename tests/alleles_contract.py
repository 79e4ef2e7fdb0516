"""The alleles contract of include/ribbit_hip.h as a plain statement: the cell of a summed amplicon, a marker's record over its
column of the genotype matrix (He and PIC from their definitions, in fractions), the refusals, both texts.  Nothing here knows the
closed forms t^2 - Q and t^4 - t^2 Q - Q^2 + F that the library computes."""
from fractions import Fraction

import primer_products_contract as prc
import primers_contract as pc

E_ARG = -1
MAX_SAMPLES, MAX_MARKERS = 1024, 1 << 24
FIELDS = ("typed", "absent", "several", "over", "alleles", "min_size", "max_size", "major_size", "major_count", "same", "off_step", "reserved", "het_num", "pic_num")
ZEROS = (0,) * 14


class Refused(Exception):
    """what the library answers with RIBBIT_E_ARG; `index` is the number its text names"""

    def __init__(self, index):
        super().__init__(index)
        self.index = index


def cell_of(amplicon, has_pair=True) -> int:
    """amplicon: a tuple of amplicons_contract.FIELDS, summed over the sample's records"""
    products = amplicon[4]
    if not has_pair or products == 0:
        return 0
    if products == 1:
        assert amplicon[7] - amplicon[6] > 0
        return amplicon[7] - amplicon[6]
    return -1 if products > 1 else -2


def marker(column, designed: int, motif_length: int):
    """one marker over its cells, one per sample -> a tuple of FIELDS"""
    if designed <= 0:
        return ZEROS
    sizes = [c for c in column if c > 0]
    t = len(sizes)
    kinds = (t, sum(1 for c in column if c == 0), sum(1 for c in column if c == -1), sum(1 for c in column if c == -2))
    assert sum(kinds) == len(column)
    same = sum(1 for c in sizes if c == designed)
    off_step = sum(1 for c in sizes if (c - designed) % motif_length != 0)
    if t == 0:
        return kinds + (0, 0, 0, 0, 0, same, off_step, 0, 0, 0)
    distinct = sorted(set(sizes))
    count = {a: sizes.count(a) for a in distinct}
    p = [Fraction(count[a], t) for a in distinct]
    he = 1 - sum(x * x for x in p)
    pic = he - sum(2 * p[i] ** 2 * p[j] ** 2 for i in range(len(p)) for j in range(i + 1, len(p)))
    het_num, pic_num = he * t ** 2, pic * t ** 4
    assert het_num.denominator == 1 and pic_num.denominator == 1
    most = max(count.values())
    major = min(a for a in distinct if count[a] == most)
    return kinds + (len(distinct), distinct[0], distinct[-1], major, most, same, off_step, 0, int(het_num), int(pic_num))


def marker_alleles(cells, designed, motif_lengths):
    """cells: S rows of n cells -> n tuples of FIELDS; the refusals in the library's order"""
    S, n = len(cells), len(designed)
    if not 1 <= S <= MAX_SAMPLES:
        raise Refused(S)
    if n > MAX_MARKERS:
        raise Refused(n)
    for i, m in enumerate(motif_lengths):
        if m < 1:
            raise Refused(i)
    for s, row in enumerate(cells):
        assert len(row) == n
        for i, c in enumerate(row):
            if c < -2:
                raise Refused(s * n + i)
    return [marker([int(cells[s][i]) for s in range(S)], int(designed[i]), int(motif_lengths[i])) for i in range(n)]


def four_decimals(ratio: Fraction) -> str:
    """rounded half up"""
    v = int(ratio * 10000 + Fraction(1, 2))      # (not negative: int() is the floor)
    return f"{v // 10000}.{v % 10000:04d}"


def _lines(bed: str):
    return bed.split("\n")[:-1] if bed.endswith("\n") else (bed.split("\n") if bed else [])


def alleles_lines(bed: str, pairs, rows, n_samples: int) -> str:
    """every line of `bed` with its 23 columns; pairs: rows of 32 values (primer_pairs_contract.FIELDS), rows: tuples of FIELDS"""
    lines = _lines(bed)
    assert len(lines) == len(pairs) == len(rows)
    out = []
    for line, r, a in zip(lines, pairs, rows):
        if r[0] < 0 or r[6] < 0:
            cols = ["."] * 23
        else:
            a_letters, b_letters = prc.oligos_of(r)
            cols = [str(r[0]), str(r[0] + r[1]), a_letters, pc.tenths(r[2]), str(r[6]), str(r[6] + r[7]), b_letters, pc.tenths(r[8]), str(r[14])]
            v = dict(zip(FIELDS, a))
            t = v["typed"]
            dot = lambda x: str(x) if t > 0 else "."
            cols += [str(n_samples), str(t), str(v["absent"]), str(v["several"]), str(v["over"]), str(v["alleles"]), dot(v["min_size"]), dot(v["max_size"]),
                     dot(v["major_size"]), str(v["major_count"]), str(v["same"]), str(v["off_step"])]
            cols += [four_decimals(Fraction(v["het_num"], t ** 2)), four_decimals(Fraction(v["pic_num"], t ** 4))] if t > 0 else [".", "."]
        out.append(line + "".join("\t" + c for c in cols) + "\n")
    return "".join(out)


FIELD_OF = {0: ".", -1: "+", -2: "*"}


def matrix_lines(bed: str, cells, designed, names) -> str:
    lines = _lines(bed)
    assert len(lines) == len(designed) and len(cells) == len(names)
    out = ["\t".join(["#name", "start", "end", "motif", "designed"] + list(names)) + "\n"]
    for i, line in enumerate(lines):
        c = line.split("\t")
        head = "\t".join(["\t".join(c[:-10])] + c[-10:-7])      # (a name may hold a tab: the row is read from the right)
        fields = [str(int(row[i])) if row[i] > 0 else FIELD_OF[int(row[i])] for row in cells]
        out.append("\t".join([head, str(int(designed[i])) if designed[i] > 0 else "."] + fields) + "\n")
    return "".join(out)


# ---- the pinned values: (cells, designed, motif_length) -> FIELDS, and the text's He and PIC
PINNED = {
    "A": ((100, 100, 100, 100), 100, 2, (4, 0, 0, 0, 1, 100, 100, 100, 4, 4, 0, 0, 0, 0), ("0.0000", "0.0000")),
    "B": ((100, 104), 100, 2, (2, 0, 0, 0, 2, 100, 104, 100, 1, 1, 0, 0, 2, 6), ("0.5000", "0.3750")),
    "C": ((100, 102, 102, 105, 0, -1, -2), 100, 2, (4, 1, 1, 1, 3, 100, 105, 102, 2, 1, 1, 0, 10, 142), ("0.6250", "0.5547")),
    "D": ((100, 102, 104, 106), 100, 2, (4, 0, 0, 0, 4, 100, 106, 100, 1, 1, 0, 0, 12, 180), ("0.7500", "0.7031")),
    "E": ((0, 0, 0), 100, 2, (0, 3, 0, 0) + (0,) * 10, (".", ".")),
    "F": ((100, 102, 0, -1), -1, 2, ZEROS, None),
}
