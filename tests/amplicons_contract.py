"""The plain statement of the amplicon contract (include/ribbit_hip.h): a primer pair typed on any record -- the sites of its two
oligos, its products, the first of them and the longest tract of its motif inside that one -- the sum over records and the marker
text.  Built on primer_products_contract.oligo_sites; the tract is the brute form: every phase of both strands, letter by
letter.  The pinned values of the contract are here too."""
import primer_pairs_contract as pp
import primer_products_contract as prc
import primers_contract as pc

FIELDS = ("left_forward", "left_reverse", "right_forward", "right_reverse", "products", "record", "start", "end", "forward_of", "reverse_of",
          "inner_start", "inner_end", "tract_start", "tract_end", "tract_strand", "reserved")
NONE = (-1, -1, -1, 0, 0, -1, -1, -1, -1, 0, 0)      # record .. reserved without a product
NO_PAIR = (0, 0, 0, 0, 0) + NONE
INT32_MAX = 2**31 - 1


def tract(letters: str, inner_start: int, inner_end: int, motif: str):
    """-> (tract_start, tract_end, tract_strand): the longest stretch of letters[inner_start:inner_end] of at least two units that
    reads as `motif` repeated at some phase (strand 0), or as its reverse complement repeated (strand 1)"""
    m = len(motif)
    best = None      # (-length, start, strand): the least wins
    for strand, w in enumerate((motif, pp.reverse_complement(motif))):
        for phase in range(m):
            s = inner_start
            for x in range(inner_start, inner_end + 1):
                if x < inner_end and letters[x] == w[(phase + x - inner_start) % m]:
                    continue
                if x - s >= 2 * m:
                    best = min(best or (0, 0, 0), (s - x, s, strand))
                s = x + 1
    return (best[1], best[1] - best[0], best[2]) if best else (-1, -1, 0)


def pair_amplicon(record, a: str, b: str, motif: str, label=0, prm=None):
    """-> the 16 values of FIELDS for the left primer a and the right primer b, both 5' to 3'"""
    prm = prm or prc.DEFAULTS
    letters = record if isinstance(record, str) else prc.letters_of(record)
    fa, va = prc.oligo_sites(letters, a, prm["seed"], prm["max_mismatches"])
    fb, vb = prc.oligo_sites(letters, b, prm["seed"], prm["max_mismatches"])
    counts = (len(fa), len(va), len(fb), len(vb))
    if max(counts) > prm["max_sites"]:
        return counts + (-1,) + NONE
    forward = [(x, len(a), 0) for x in fa] + [(x, len(b), 1) for x in fb]
    reverse = [(x, len(a), 0) for x in va] + [(x, len(b), 1) for x in vb]
    products = [(fx, vx + vk, f_of, v_of, fx + fk, vx) for fx, fk, f_of in forward for vx, vk, v_of in reverse
                if fx + fk <= vx and vx + vk - fx <= prm["max_product"]]
    if not products:
        return counts + (0,) + NONE
    first = min(products)
    return counts + (len(products), label) + first + tract(letters, first[4], first[5], motif) + (0,)


def record_pair_amplicons(record: bytes, pairs, motifs, label=0, prm=None):
    """pairs: rows of 32 values (primer_pairs_contract.FIELDS) -> one tuple of FIELDS each"""
    letters, out, seen = prc.letters_of(record), [], {}
    for r, motif in zip(pairs, motifs):
        if r[0] < 0:
            out.append(NO_PAIR)
            continue
        key = prc.oligos_of(r) + (motif,)
        if key not in seen:
            seen[key] = pair_amplicon(letters, *key, label, prm)
        out.append(seen[key])
    return out


def merge(into, other):
    """the sum of two tuples of FIELDS"""
    sat = lambda x, y: min(x + y, INT32_MAX)
    counts = tuple(sat(x, y) for x, y in zip(into[:4], other[:4]))
    products = -1 if -1 in (into[4], other[4]) else sat(into[4], other[4])
    if products <= 0:
        return counts + (products,) + NONE
    return counts + (products,) + (into[5:] if into[4] > 0 else other[5:])


def genome_amplicons(genome, pairs, motifs, prm=None):
    """the pairs typed on every record of `genome` (a list of bytes), merged in record order"""
    total = None
    for k, bases in enumerate(genome):
        here = record_pair_amplicons(bases, pairs, motifs, k, prm)
        total = here if total is None else [merge(t, h) for t, h in zip(total, here)]
    return total if total is not None else [NO_PAIR if r[0] < 0 else (0, 0, 0, 0, 0) + NONE for r in pairs]


ORIENTATION = {(0, 1): "+", (1, 0): "-", (0, 0): "l", (1, 1): "r"}


def marker_lines(bed: str, pairs, amplicons, names) -> str:
    """every line of `bed` with its 20 marker columns"""
    lines = bed.split("\n")[:-1] if bed.endswith("\n") else (bed.split("\n") if bed else [])
    assert len(lines) == len(pairs) == len(amplicons)
    out = []
    for line, r, a in zip(lines, pairs, amplicons):
        if r[0] < 0 or r[6] < 0:
            cols = ["."] * 20
        else:
            a_letters, b_letters = prc.oligos_of(r)
            cols = [str(r[0]), str(r[0] + r[1]), a_letters, pc.tenths(r[2]), str(r[6]), str(r[6] + r[7]), b_letters, pc.tenths(r[8]), str(r[14])]
            cols.append("." if a[4] < 0 else str(a[4]))
            if a[4] != 1:
                cols += ["."] * 10
            else:
                size = a[7] - a[6]
                cols += [names[a[5]], str(a[6]), str(a[7]), ORIENTATION[(a[8], a[9])], str(size), str(size - r[14])]
                if a[12] < 0:
                    cols += ["."] * 4
                else:
                    m = len(line.split("\t")[-8])
                    cols += [str(a[12]), str(a[13]), str(a[13] - a[12]), str((a[13] - a[12]) // m)]
        out.append(line + "".join("\t" + c for c in cols) + "\n")
    return "".join(out)


def as_tuples(arr):
    return [tuple(int(v) for v in r) for r in arr.tolist()]


# ---- the pinned values: (record, motif) -> the four counts, products, (start .. tract_strand); a = Lp, b = revcomp(Rp), the defaults
LP, RP = "GATTACAGATTACAGGCT", "CCTGAAGTCTCGGATCAA"
A, B = LP, pp.reverse_complement(RP)
X, Y = "ACGTTGCATG", "CCATGACTGA"
REC = LP + X + "CA" * 10 + Y + RP
PINNED = {
    (REC, "CA"): ((1, 0, 0, 1), 1, (0, 76, 0, 1, 18, 58, 28, 49, 0)),      # the tract takes Y's first C
    (REC, "AC"): ((1, 0, 0, 1), 1, (0, 76, 0, 1, 18, 58, 28, 49, 0)),
    (REC, "TG"): ((1, 0, 0, 1), 1, (0, 76, 0, 1, 18, 58, 28, 49, 1)),
    (pp.reverse_complement(REC), "CA"): ((0, 1, 1, 0), 1, (0, 76, 1, 0, 18, 58, 27, 48, 1)),
    (LP + X + "CA" * 17 + Y + RP, "CA"): ((1, 0, 0, 1), 1, (0, 90, 0, 1, 18, 72, 28, 63, 0)),
    (LP + X + "CA" * 4 + "N" + "CA" * 5 + Y + RP, "CA"): ((1, 0, 0, 1), 1, (0, 75, 0, 1, 18, 57, 37, 48, 0)),
    (LP + X + "CA" + Y + RP, "CA"): ((1, 0, 0, 1), 1, (0, 58, 0, 1, 18, 40, -1, -1, 0)),
    (REC.lower(), "CA"): ((1, 0, 0, 1), 1, (0, 76, 0, 1, 18, 58, 28, 49, 0)),
    (REC + "ACGTAGCTAGCTAGGATCGA" + REC, "CA"): ((2, 0, 0, 2), 3, (0, 76, 0, 1, 18, 58, 28, 49, 0)),
    (LP + "GATA" * 6 + RP, "ATAG"): ((1, 0, 0, 1), 1, (0, 60, 0, 1, 18, 42, 18, 42, 0)),
    (LP + X, "CA"): ((1, 0, 0, 0), 0, None),
}


def pinned_fields(value, label=0):
    counts, products, placed = value
    return counts + (products,) + ((label,) + placed + (0,) if placed else NONE)
