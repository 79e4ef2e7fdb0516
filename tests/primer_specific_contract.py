"""The plain statement of the specific primer pair contract (include/ribbit_hip.h): the shortlists and the admissible pairs of a
target are primer_pairs_contract's (`side`, `duplex`), the pairs are put into the order of its choice, each is judged by
primer_products_contract's `pair_products`, and the first specific one is taken.  Nothing here is shared with the library.  The
five constructed records whose values the header pins are here too, and the text formatter."""
import primer_pairs_contract as pp
import primer_products_contract as pq
import primers_contract as pc

FIELDS = ("place", "pairs_admissible", "pairs_specific", "pairs_over", "pairs_other", "first_products", "reserved0", "reserved1")


def ordered_pairs(left, right, pair, duplex_of=pp.duplex):
    """the admissible pairs of two shortlists (primer_pairs_contract.side's entries) in the order of the choice:
    (key, a, b, Tm difference, pair any, pair end)"""
    out = []
    for l, a in enumerate(left):
        for r, b in enumerate(right):
            difference = abs(a[2] - b[2])
            if difference > pair["max_tm_difference"]:
                continue
            pair_any, pair_end = duplex_of(a[3], b[3])
            if pair_any > pair["max_pair_any"] or pair_end > pair["max_pair_end"]:
                continue
            out.append(((a[0][0] + b[0][0] + difference, b[1] + b[0][2] - a[1], l, r), a, b, difference, pair_any, pair_end))
    out.sort(key=lambda entry: entry[0])
    return out


def choose_specific(letters: str, left, right, counts, pair, product, duplex_of=pp.duplex):
    """-> (the 32 values of the pair record, the 8 of its products, the 8 of the summary) of one target"""
    ordered = ordered_pairs(left, right, pair, duplex_of)
    tail = counts + (len(left) * len(right), len(ordered), 0)
    place, chosen, specific, over, other, first = -1, None, 0, 0, 0, 0
    for at, entry in enumerate(ordered):
        a, b = entry[1], entry[2]
        # a is the left candidate's oligo, b the right one's as ordered; own is (a forward at a's start, b reverse at b's start)
        found = pq.pair_products(letters, a[3], b[3], a[1], b[1], product)
        if at == 0:
            first = -1 if found[4] == -1 else found[4] - found[5]
        if found[4] == -1:
            over += 1
        elif found[4] - found[5] == 0:
            specific += 1
            if chosen is None:
                place, chosen = at, (entry, found)
        else:
            other += 1
    summary = (place, len(ordered), specific, over, other, first, 0, 0)
    if chosen is None:
        return pc.NO_PRIMER * 2 + (0,) * 13 + tail, pq.NO_PRODUCTS, summary
    (key, a, b, difference, pair_any, pair_end), found = chosen
    record = (pp._primer(letters, a[1], a[0][2], a[2], a[0][0]) + pp._primer(letters, b[1], b[0][2], b[2], b[0][0]) + (key[0], difference, key[1], key[2], key[3])
              + a[4:7] + b[4:7] + (pair_any, pair_end) + tail)
    return record, found, summary


class _SitesOnce:
    """primer_products_contract.pair_products looks the sites of both oligos up again for every pair; within one record and one set of
    parameters the 16 oligos of a target, and on tiled records those of many targets, are the same few.  While this is entered,
    every (oligo, seed, max_mismatches) is searched once with the plain function and answered from a dictionary after that."""

    def __enter__(self):
        self.plain, seen = pq.oligo_sites, {}

        def once(record, oligo, seed=15, max_mismatches=2):
            key = (oligo, seed, max_mismatches)
            if key not in seen:
                seen[key] = self.plain(record, oligo, seed, max_mismatches)
            return seen[key]

        pq.oligo_sites = once

    def __exit__(self, *exc):
        pq.oligo_sites = self.plain


def record_specific_primer_pairs(seq: bytes, rows, targets, prm=None, pair=None, product=None, loops=True):
    """-> (pairs, products, summaries), one tuple per target each.  loops=False: the shortlists from primer_pairs_contract's
    arrays and the duplex on packed oligos, for the larger cases (both forms are tested against each other there)"""
    prm, pair, product = prm or pc.DEFAULTS, pair or pp.PAIR_DEFAULTS, product or pq.DEFAULTS
    letters = seq.decode("latin-1").upper()
    blocked = pc.blocked_positions(seq, rows) if loops else None
    arrays = None if loops else pp.PairArrays(seq, rows, prm, pair)
    pairs, products, summaries = [], [], []
    with _SitesOnce():
        for s, e in [(int(s), int(e)) for s, e in targets]:
            s1, e1, lo, hi = pc.clip(s, e, prm["flank"], len(seq))
            if loops:
                left, n_left, p_left = pp.side(letters, blocked, lo, s1, False, prm, pair)
                right, n_right, p_right = pp.side(letters, blocked, e1, hi, True, prm, pair)
            else:
                left, n_left, p_left = arrays.shortlist(lo, s1, False)
                right, n_right, p_right = arrays.shortlist(e1, hi, True)
            record, found, summary = choose_specific(letters, left, right, (n_left, n_right, p_left, p_right), pair, product, pp.duplex if loops else pp.duplex_packed)
            pairs.append(record)
            products.append(found)
            summaries.append(summary)
    return pairs, products, summaries


def as_tuples(arr):
    return [tuple(int(v) for v in r) for r in arr.tolist()]


# ---- the text
def specific_lines(bed: str, pairs, products, summaries) -> str:
    lines = pq.product_lines(bed, pairs, products).split("\n")[:-1] if len(pairs) else []
    assert len(lines) == len(summaries)
    return "".join(line + "\t" + "\t".join(["." if s[0] < 0 else str(s[0]), str(s[2]), str(s[3]), str(s[4])]) + "\n" for line, s in zip(lines, summaries))


# ---- the five constructed records: 4,000 random bases with (CA)20 at 1500, the target (1500, 1540), no rows
TARGET = (1500, 1540)


def _put(seq: bytes, at: int, part: bytes) -> bytes:
    return seq[:at] + part + seq[at + len(part):]


def base_record() -> bytes:
    return _put(pc.clean_record(4000, 1).upper(), TARGET[0], b"CA" * 20)


def constructed():
    """name -> (record, the product parameters that differ from the defaults)"""
    plain = base_record()
    best = pp.record_primer_pairs(plain, [], [TARGET])[0]
    left, right = plain[best[0]:best[0] + best[1]], plain[best[6]:best[6] + best[7]]
    # the best pair's two windows a second time, 60 bases between them: that pair has a second product there
    copied = _put(_put(plain, 3000, left), 3000 + len(left) + 60, right)
    both = _put(_put(plain, 2600, plain[1300:1500]), 2800, plain[1540:1740])
    left_only = _put(plain, 2600, plain[1300:1500])
    return {"undisturbed": (plain, {}), "best pair copied": (copied, {}), "both flanks copied": (both, {}), "left flank copied": (left_only, {}),
            "left flank copied, max_sites 1": (left_only, {"max_sites": 1})}


# name -> the summary's first six values, and (left start, left length, right start, right length) of the chosen pair; computed
# with this file, written into include/ribbit_hip.h
PINNED = {
    "undisturbed": ((0, 44, 44, 0, 0, 0), (1304, 22, 1624, 21)),
    "best pair copied": ((2, 44, 26, 0, 18, 2), (1304, 22, 1613, 22)),
    "both flanks copied": ((-1, 44, 0, 0, 44, 2), (-1, 0, -1, 0)),
    "left flank copied": ((0, 44, 44, 0, 0, 0), (1304, 22, 1624, 21)),
    "left flank copied, max_sites 1": ((-1, 44, 0, 44, 0, -1), (-1, 0, -1, 0)),
}
