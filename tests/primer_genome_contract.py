"""The plain statement of the genome-wide specific primer pair contract (include/ribbit_hip.h), written on top of the three contract
modules it sits on: a target's shortlists and its admissible pairs in order are primer_specific_contract's (made on the home record
against the home record's rows), every pair is judged by primer_products_contract's `pair_products` on every record of the genome,
with the own positions on the home record alone, and the judgements are summed: over on any record is over, else others above 0 is
other, else specific.  Nothing here is shared with the library.  The three genomes whose values the header pins are here too."""
import primer_pairs_contract as pp
import primer_products_contract as pq
import primer_specific_contract as ps
import primers_contract as pc

VERDICT_FIELDS = ("admissible", "over", "other", "own", "forward", "reverse", "first_others", "records", "home_records", "reserved")


class _SitesOncePerRecord:
    """as primer_specific_contract._SitesOnce, for several records: every (record, oligo, seed, max_mismatches) is searched once with
    the plain function.  The records are told apart by their letters' identity, so the caller keeps them alive."""

    def __enter__(self):
        self.plain, seen = pq.oligo_sites, {}

        def once(record, oligo, seed=15, max_mismatches=2):
            key = (id(record), oligo, seed, max_mismatches)
            if key not in seen:
                seen[key] = (record, self.plain(record, oligo, seed, max_mismatches))
            return seen[key][1]

        pq.oligo_sites = once

    def __exit__(self, *exc):
        pq.oligo_sites = self.plain


def target_shortlists(seq: bytes, rows, targets, prm=None, pair=None, loops=True):
    """-> per target (left, right, (left_candidates, right_candidates, left_passed, right_passed)), the two lists as
    primer_pairs_contract.side gives them"""
    prm, pair = prm or pc.DEFAULTS, pair or pp.PAIR_DEFAULTS
    letters = seq.decode("latin-1").upper()
    blocked = pc.blocked_positions(seq, rows) if loops else None
    arrays = None if loops else pp.PairArrays(seq, rows, prm, pair)
    out = []
    for s, e in [(int(s), int(e)) for s, e in targets]:
        s1, e1, lo, hi = pc.clip(s, e, prm["flank"], len(seq))
        if loops:
            left, n_left, p_left = pp.side(letters, blocked, lo, s1, False, prm, pair)
            right, n_right, p_right = pp.side(letters, blocked, e1, hi, True, prm, pair)
        else:
            left, n_left, p_left = arrays.shortlist(lo, s1, False)
            right, n_right, p_right = arrays.shortlist(e1, hi, True)
        out.append((left, right, (n_left, n_right, p_left, p_right)))
    return out


def shortlists_as_tuples(seq: bytes, lists):
    """target_shortlists' result as the 100 values of a RibbitTargetShortlists each: 8 + 8 primers of 6 values by rank, an empty
    place (-1, 0, 0, 0, 0, 0), then the four counts"""
    letters = seq.decode("latin-1").upper()
    out = []
    for left, right, counts in lists:
        flat = ()
        for side in (left, right):
            for rank in range(8):
                flat += pp._primer(letters, side[rank][1], side[rank][0][2], side[rank][2], side[rank][0][0]) if rank < len(side) else pc.NO_PRIMER
        out.append(flat + counts)
    return out


def record_verdicts(letters: str, left, right, home: bool, pair=None, product=None, duplex_of=pp.duplex):
    """one target's judgement on one record -> the ten values of VERDICT_FIELDS, forward and reverse as tuples of 16"""
    pair, product = pair or pp.PAIR_DEFAULTS, product or pq.DEFAULTS
    ordered = ps.ordered_pairs(left, right, pair, duplex_of)
    admissible = over = other = own = first = 0
    for at, (key, a, b, _, _, _) in enumerate(ordered):
        bit = 1 << (8 * key[2] + key[3])
        found = pq.pair_products(letters, a[3], b[3], a[1] if home else -1, b[1] if home else -1, product)
        admissible |= bit
        others = -1 if found[4] == -1 else found[4] - found[5]
        over |= bit if others == -1 else 0
        other |= bit if others > 0 else 0
        own |= bit if found[5] else 0
        if at == 0:
            first = others
    forward, reverse = [0] * 16, [0] * 16
    for slot, entry in [(rank, e) for rank, e in enumerate(left)] + [(8 + rank, e) for rank, e in enumerate(right)]:
        f, v = pq.oligo_sites(letters, entry[3], product["seed"], product["max_mismatches"])
        forward[slot], reverse[slot] = len(f), len(v)
    return admissible, over, other, own, tuple(forward), tuple(reverse), first, 1, int(home), 0


def merge(a, b):
    """the sum of two judgements of one target (without the saturation, which no test record reaches)"""
    assert a[0] == b[0]
    return (a[0], a[1] | b[1], a[2] | b[2], a[3] | b[3], tuple(x + y for x, y in zip(a[4], b[4])), tuple(x + y for x, y in zip(a[5], b[5])),
            -1 if -1 in (a[6], b[6]) else a[6] + b[6], a[7] + b[7], a[8] + b[8], 0)


def choose(letters: str, left, right, counts, verdicts, pair=None, duplex_of=pp.duplex):
    """-> (the 32 values of the pair record, the 8 of its products, the 8 of the summary) of one target from its summed judgement"""
    pair = pair or pp.PAIR_DEFAULTS
    admissible, over, other, own, forward, reverse, first = verdicts[:7]
    ordered = ps.ordered_pairs(left, right, pair, duplex_of)
    tail = counts + (len(left) * len(right), len(ordered), 0)
    n_over, n_other = bin(over).count("1"), bin(other & ~over).count("1")
    chosen = next((at for at, entry in enumerate(ordered) if not (over | other) >> (8 * entry[0][2] + entry[0][3]) & 1), -1)
    summary = (chosen, len(ordered), len(ordered) - n_over - n_other, n_over, n_other, first, 0, 0)
    if chosen < 0:
        return pc.NO_PRIMER * 2 + (0,) * 13 + tail, pq.NO_PRODUCTS, summary
    key, a, b, difference, pair_any, pair_end = ordered[chosen]
    record = (pp._primer(letters, a[1], a[0][2], a[2], a[0][0]) + pp._primer(letters, b[1], b[0][2], b[2], b[0][0]) + (key[0], difference, key[1], key[2], key[3])
              + a[4:7] + b[4:7] + (pair_any, pair_end) + tail)
    is_own = own >> (8 * key[2] + key[3]) & 1
    return record, (forward[key[2]], reverse[key[2]], forward[8 + key[3]], reverse[8 + key[3]], is_own, is_own, 0, 0), summary


def genome_specific_primer_pairs(records, home: int, rows, targets, prm=None, pair=None, product=None, loops=True):
    """records: the genome in input order; rows and targets lie on records[home] -> (pairs, products, summaries), one tuple per
    target each, as primer_specific_contract.record_specific_primer_pairs gives them for one record"""
    prm, pair, product = prm or pc.DEFAULTS, pair or pp.PAIR_DEFAULTS, product or pq.DEFAULTS
    letters = [pq.letters_of(r) for r in records]
    duplex_of = pp.duplex if loops else pp.duplex_packed
    pairs, products, summaries = [], [], []
    with _SitesOncePerRecord():
        for left, right, counts in target_shortlists(records[home], rows, targets, prm, pair, loops):
            total = None
            for k, record in enumerate(letters):
                one = record_verdicts(record, left, right, k == home, pair, product, duplex_of)
                total = one if total is None else merge(total, one)
            assert total[7:9] == (len(records), 1)
            record, found, summary = choose(letters[home], left, right, counts, total, pair, duplex_of)
            pairs.append(record)
            products.append(found)
            summaries.append(summary)
    return pairs, products, summaries


# ---- the three pinned genomes: R0 is primer_specific_contract's undisturbed record with the target (1500, 1540), no rows; R1 is B,
# 4,000 other random bases, as it stands or with parts of R0 put into it
TARGET = ps.TARGET


def other_record() -> bytes:
    return pc.clean_record(4000, 2).upper()


def pinned_genomes():
    """name -> (R0, R1)"""
    home, plain = ps.base_record(), other_record()
    best = pp.record_primer_pairs(home, [], [TARGET])[0]
    left, right = home[best[0]:best[0] + best[1]], home[best[6]:best[6] + best[7]]
    copied = ps._put(ps._put(plain, 3000, left), 3000 + len(left) + 60, right)
    both = ps._put(ps._put(plain, 2600, home[1300:1500]), 2800, home[1540:1740])
    return {"undisturbed": (home, plain), "best pair copied to the other record": (home, copied), "both flanks copied to the other record": (home, both)}


# name -> the summary's first six values, and (left start, left length, right start, right length) of the chosen pair; computed
# with this file, written into include/ribbit_hip.h
PINNED = {
    "undisturbed": ((0, 44, 44, 0, 0, 0), (1304, 22, 1624, 21)),
    "best pair copied to the other record": ((2, 44, 30, 0, 14, 1), (1304, 22, 1613, 22)),
    "both flanks copied to the other record": ((-1, 44, 0, 0, 44, 1), (-1, 0, -1, 0)),
}
