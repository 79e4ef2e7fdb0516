"""What tests/test_panel.py and tests/test_panel_gpu.py share: seeded random panels, the properties every answer has, and the
records, the derived second assembly and the parsers of the tool's end-to-end run."""
import numpy as np

import panel_contract as pc
import primer_pairs_contract as pp
from ribbit_amd.simulate import _mutate, _primitive_motif


def random_oligo(rs, k=None):
    return "".join(rs.choice(list("ACGT"), k or rs.randint(15, 33)))


def random_panel(n, rs, none_every=7, groups=3, lengths=(15, 33)):
    """n rows: oligos of lengths[0] .. lengths[1] - 1 bases (the first two pairs have 15 and 32 on either side), every none_every-th
    row or so without a pair; starts within 12,000 bases and `groups` groups, so that the near rule meets both answers; sizes
    80 .. 400 with ranges of up to 25 around them -> (pairs, extra)"""
    pairs, extra = [], []
    for i in range(n):
        if i >= 2 and rs.randint(none_every) == 0:
            pairs.append(pc.NO_PAIR)
            extra.append((int(rs.randint(-1, groups)), 5, 5))
            continue
        a = random_oligo(rs, (15, 32)[i] if i < 2 else rs.randint(*lengths))
        b = random_oligo(rs, (32, 15)[i] if i < 2 else rs.randint(*lengths))
        start, product = int(rs.randint(0, 12000)), int(rs.randint(80, 400))
        pairs.append(pc.pair(a, b, start, start + product - len(b)))
        extra.append((int(rs.randint(-1, groups)), product - int(rs.randint(0, 13)), product + int(rs.randint(0, 13))))
    return pairs, extra


def sparse_panel(n, rs, dense=(), one_in=7, lengths=(15, 33)):
    """n rows of which one in `one_in` has a pair, and every row of `dense` has: the twin stays quick, and the kernel still takes
    every tile and chunk"""
    pairs, extra = random_panel(n, rs, none_every=1 << 30, lengths=lengths)
    keep = rs.randint(one_in, size=n) == 0
    keep[list(dense)] = True
    return [p if k else pc.NO_PAIR for p, k in zip(pairs, keep)], extra


def check_properties(pairs, rows, pools, pool_size):
    sizes = [0] * pools
    for pair, r in zip(pairs, rows):
        assert r[5:] == (0, 0, 0)
        if not pc.has_pair(pair):
            assert r == pc.NOT_POOLED
            continue
        assert 0 <= r[0] < pools and max(r[2:5]) <= r[1] <= sum(r[2:5])
        sizes[r[0]] += 1
    assert all(0 < s <= pool_size for s in sizes)


# ---- the tool's end-to-end run
def three_records():
    """three records of about 20 kb: 30 loci each as the simulator makes them (motifs of 2 .. 8 bases, 85 to 95 % pure), 450 .. 700
    random bases between them and an N block before one in five"""
    made = []
    for k in range(3):
        rs = np.random.RandomState(900 + k)
        parts = []
        for _ in range(30):
            parts.append(bytes(rs.choice(list(b"ACGT"), rs.randint(450, 701)).tolist()))
            if rs.random_sample() < 0.2:
                parts.append(b"N" * rs.randint(1, 201))
            m = int(rs.randint(2, 9))
            units = int(rs.randint(8, 25))
            parts.append(_mutate(rs, _primitive_motif(rs, m) * units, m, units, 0.85, 0.95))
        parts.append(bytes(rs.choice(list(b"ACGT"), 500).tolist()))
        made.append((f"home{k}", b"".join(parts)))
    return made


def primer_row(c):
    """the row of 32 values of a line's columns 12 .. 20 (the eight primer columns and the designed product), or None without a pair"""
    if c[11] == ".":
        return None
    row = ()
    for start, end, letters, tm, right in ((c[11], c[12], c[13], c[14], False), (c[15], c[16], c[17], c[18], True)):
        forward = pp.reverse_complement(letters) if right else letters
        bases = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(forward))
        row += (int(start), int(end) - int(start), int(tm.replace(".", "")), 0, pp._i32(bases & 0xffffffff), pp._i32(bases >> 32))
    return row + (0, 0, int(c[19])) + (0,) * 17


def second_assembly(home, genome_bed: str):
    """the home records as another individual's: of the rows of --primer-genome-bed that have a pair, record by record, one in four
    keeps its length, one loses one to three units and two gain as many in their middle; the records change places"""
    made = []
    for name, bases in home:
        rows = [c for c in (l.split("\t") for l in genome_bed.splitlines()) if c[0] == name and c[11] != "."]
        seq = bytearray(bases)
        for j, c in reversed(list(enumerate(rows))):      # (from the right, so that the positions to the left stay)
            s, e, motif = int(c[1]), int(c[2]), c[3]
            k, m, mid = 1 + j % 3, len(c[3]), (int(c[1]) + int(c[2])) // 2
            if j % 4 == 3:
                continue
            if j % 4 == 2:
                if e - s > k * m + 2 * m:
                    del seq[mid:mid + k * m]
                continue
            seq[mid:mid] = (motif * k).encode()
        made.append(("other" + name[4:], bytes(seq)))
    return made[::-1]


def marker_rows(marker_text: str, names):
    """the lines of --marker-bed as (the row of 32 values or None, the home record's index, products, observed size or None, the line)"""
    out = []
    for line in marker_text.splitlines():
        c = line.split("\t")
        assert len(c) == 31
        out.append((primer_row(c), names.index(c[0]), c[20], int(c[25]) if c[20] == "1" else None, line))
    return out
