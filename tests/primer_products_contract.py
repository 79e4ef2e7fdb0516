"""The plain statement of the in-silico PCR contract (include/ribbit_hip.h): the sites of an oligo on either strand of a record,
the products of a primer pair among them, and the text.  Everything is over letters: a `str.find` brings up the places where the
seed matches, a loop over letters judges the window.  The pinned values of the contract are here too."""
import primer_pairs_contract as pp
import primers_contract as pc

DEFAULTS = dict(seed=15, max_mismatches=2, max_product=4000, max_sites=64)
FIELDS = ("left_forward", "left_reverse", "right_forward", "right_reverse", "products", "own", "shortest_other", "reserved")
NO_PRODUCTS = (0,) * 8


def params(**fields):
    assert set(fields) <= set(DEFAULTS)
    return dict(DEFAULTS, **fields)


def letters_of(record: bytes) -> str:
    """the record with case ignored; every byte that is not a base stays what it is, so it matches no oligo"""
    return record.decode("latin-1").upper()


def _found(letters: str, part: str):
    at = letters.find(part)
    while at >= 0:
        yield at
        at = letters.find(part, at + 1)


def oligo_sites(record, oligo: str, seed=15, max_mismatches=2):
    """-> (forward, reverse): the ascending window starts x of the sites of `oligo` (5' to 3') on the two strands"""
    letters = record if isinstance(record, str) else letters_of(record)
    o = oligo.upper()
    k, q = len(o), pp.reverse_complement(oligo.upper())
    assert seed <= k <= 32 and set(o) <= set("ACGT")

    def judged(x, pattern, free):
        if x < 0 or x + k > len(letters):
            return False
        window = letters[x:x + k]
        return all(ch in "ACGT" for ch in window) and sum(window[j] != pattern[j] for j in free) <= max_mismatches

    forward = [at - (k - seed) for at in _found(letters, o[k - seed:]) if judged(at - (k - seed), o, range(k - seed))]
    reverse = [at for at in _found(letters, q[:seed]) if judged(at, q, range(seed, k))]
    return forward, reverse


def pair_products(record, a: str, b: str, left_start: int, right_start: int, prm=None):
    """-> the eight values of FIELDS for the left primer a and the right primer b, both 5' to 3'"""
    prm = prm or DEFAULTS
    fa, va = oligo_sites(record, a, prm["seed"], prm["max_mismatches"])
    fb, vb = oligo_sites(record, b, prm["seed"], prm["max_mismatches"])
    counts = (len(fa), len(va), len(fb), len(vb))
    if max(counts) > prm["max_sites"]:
        return counts + (-1, 0, 0, 0)
    forward = [(x, len(a), "a") for x in fa] + [(x, len(b), "b") for x in fb]
    reverse = [(x, len(a), "a") for x in va] + [(x, len(b), "b") for x in vb]
    products, own, others = 0, 0, []
    for fx, fk, f_of in forward:
        for vx, vk, v_of in reverse:
            size = vx + vk - fx
            if fx + fk <= vx and size <= prm["max_product"]:
                products += 1
                if (f_of, fx, v_of, vx) == ("a", left_start, "b", right_start):
                    own = 1
                else:
                    others.append(size)
    return counts + (products, own, min(others, default=0), 0)


def sites_as_lists(sites, positions):
    """-> per oligo (forward count, reverse count, forward list or None, reverse list or None), and checks where the lists lie"""
    out, at = [], 0
    for f, v, f_at, v_at in sites.tolist():
        lists = []
        for count, start in ((f, f_at), (v, v_at)):
            if start < 0:
                lists.append(None)
                continue
            assert start == at
            lists.append(positions[at:at + count].tolist())
            at += count
        out.append((f, v, lists[0], lists[1]))
    assert at == len(positions)
    return out


def contract_sites(seq, oligos, prm):
    out = []
    for o in oligos:
        f, v = oligo_sites(seq, o if isinstance(o, str) else o.decode(), prm["seed"], prm["max_mismatches"])
        out.append((len(f), len(v), f if len(f) <= prm["max_sites"] else None, v if len(v) <= prm["max_sites"] else None))
    return out


def pair_tuple(a: str, b: str, left_start: int, right_start: int):
    """a hand-made row of 32 values: the left primer a and the right primer b (as ordered, 5' to 3') at their starts, all else 0"""
    out = ()
    for letters, start in ((a, left_start), (pp.reverse_complement(b), right_start)):
        bases = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(letters))
        out += (start, len(letters), 0, 0, pp._i32(bases & 0xffffffff), pp._i32(bases >> 32))
    return out + (0,) * 20


def oligos_of(row):
    """(a, b) of a row of 32 values (primer_pairs_contract.FIELDS): the left primer, and the right primer as it is ordered"""
    return pc.oligo_of(row[:6]), pc.oligo_of(row[6:12])[::-1].translate(pc.COMPLEMENT)


def record_primer_products(record: bytes, pairs, prm=None):
    """pairs: rows of 32 values -> one tuple of FIELDS each"""
    letters, out, seen = letters_of(record), [], {}
    for r in pairs:
        if r[0] < 0:
            out.append(NO_PRODUCTS)
            continue
        key = oligos_of(r) + (r[0], r[6])
        if key not in seen:
            seen[key] = pair_products(letters, *key, prm)
        out.append(seen[key])
    return out


def as_tuples(arr):
    return [tuple(int(v) for v in r) for r in arr.tolist()]


def product_lines(bed: str, pairs, products) -> str:
    lines = pp.pair_lines(bed, pairs).split("\n")[:-1] if len(pairs) else []
    assert len(lines) == len(products)
    out = []
    for line, r, p in zip(lines, pairs, products):
        if r[0] < 0:
            cols = ["."] * 6
        else:
            cols = [str(v) for v in p[:4]] + ([".", "."] if p[4] < 0 else [str(p[4] - p[5]), str(p[6])])
        out.append(line + "".join("\t" + c for c in cols) + "\n")
    return "".join(out)


# ---- the pinned values: (record, a, b, left start, right start, parameters that differ from the defaults) -> FIELDS
_L = "GATTACAGATTACAGGCT"      # 18 bases
_R = "CCTGAAGTCTCGGATCAA"      # 18 bases; the right primer as ordered is its reverse complement
_RB = pp.reverse_complement(_R)
_MID = "ACGTTGCATGCCATGACTGA"
PALINDROME = "ACGTACGTACGTACGT"
PINNED = {
    # one product, its own
    (_L + _MID + _R, _L, _RB, 0, 38, ()): (1, 0, 0, 1, 1, 1, 0, 0),
    # a mismatch in the seed (the left primer's last base) loses the site
    (_L[:-1] + "A" + _MID + _R, _L, _RB, 0, 38, ()): (0, 0, 0, 1, 0, 0, 0, 0),
    # exactly d = 2 mismatches outside the seed, and d + 1
    ("CT" + _L[2:] + _MID + _R, _L, _RB, 0, 38, ()): (1, 0, 0, 1, 1, 1, 0, 0),
    ("CTA" + _L[3:] + _MID + _R, _L, _RB, 0, 38, ()): (0, 0, 0, 1, 0, 0, 0, 0),
    # an N in the window, outside the seed
    ("N" + _L[1:] + _MID + _R, _L, _RB, 0, 38, ()): (0, 0, 0, 1, 0, 0, 0, 0),
    # a window hanging off either end
    (_L[1:] + _MID + _R, _L, _RB, 0, 37, ()): (0, 0, 0, 1, 0, 0, 0, 0),
    (_L + _MID + _R[:-1], _L, _RB, 0, 38, ()): (1, 0, 0, 0, 0, 0, 0, 0),
    # a palindrome has both sites at one x, and a == b counts each site twice: alone no two windows are clear of each other;
    # twice in a row it has a site at every fourth x of 0 .. 16 and the four products (0, 16), one of them its own
    (PALINDROME, PALINDROME, PALINDROME, 0, 0, ()): (1, 1, 1, 1, 0, 0, 0, 0),
    (PALINDROME + PALINDROME, PALINDROME, PALINDROME, 0, 16, ()): (5, 5, 5, 5, 4, 1, 32, 0),
    # size == max_product and max_product + 1
    (_L + _MID + _R, _L, _RB, 0, 38, (("max_product", 56),)): (1, 0, 0, 1, 1, 1, 0, 0),
    (_L + _MID + _R, _L, _RB, 0, 38, (("max_product", 55),)): (1, 0, 0, 1, 0, 0, 0, 0),
    # abutting windows, and windows that overlap by one base (the left primer ends in C, the right window starts with C)
    (_L + _R, _L, _RB, 0, 18, ()): (1, 0, 0, 1, 1, 1, 0, 0),
    (_L[:-1] + "C" + _R[1:], _L[:-1] + "C", _RB, 0, 17, ()): (1, 0, 0, 1, 0, 0, 0, 0),
    # a left-left product: the left primer's reverse site downstream, nearer than the right primer's
    (_L + _MID + pp.reverse_complement(_L) + _MID + _R, _L, _RB, 0, 76, ()): (1, 1, 0, 1, 2, 1, 56, 0),
    # a list longer than max_sites: the counts stay exact
    (_L + _MID + _L + _MID + _R, _L, _RB, 0, 76, (("max_sites", 1),)): (2, 0, 0, 1, -1, 0, 0, 0),
    (_L + _MID + _L + _MID + _R, _L, _RB, 0, 76, ()): (2, 0, 0, 1, 2, 1, 56, 0),
}
