"""The plain statement of the primer pair contract (include/ribbit_hip.h), on top of primers_contract.py's windows, blocked
positions, five rules and Tm.  `duplex`, `hairpin` and `record_primer_pairs` are loops over letters that read like the contract.
For the larger cases there is a second form: oligos as Python integers, two bits a base, and per-record numpy arrays that say for
every start and length whether the candidate there passes its self limits (PairArrays).  The text formatter and the pinned values
of the contract are here too."""
import numpy as np

import primers_contract as pc
from primers_contract import admissible, blocked_positions, clip, tm_of

FIELDS = (tuple(f"{side}_{n}" for side in ("left", "right") for n in ("start", "length", "tm", "penalty", "bases_lo", "bases_hi"))
          + ("pair_penalty", "tm_difference", "product", "left_rank", "right_rank", "left_self_any", "left_self_end", "left_hairpin", "right_self_any", "right_self_end",
             "right_hairpin", "pair_any", "pair_end", "left_candidates", "right_candidates", "left_passed", "right_passed", "pairs_tried", "pairs_admissible", "reserved"))
PAIR_DEFAULTS = dict(shortlist=8, max_self_any=4, max_self_end=3, max_hairpin=3, max_pair_any=4, max_pair_end=3, max_tm_difference=30)
LOOSE = dict(shortlist=1, max_self_any=32, max_self_end=32, max_hairpin=32, max_pair_any=32, max_pair_end=32, max_tm_difference=2000)
HAIRPIN_LOOP, MAX_SHORTLIST = 3, 8
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}

# (a, b) -> (any, end), and a -> hairpin: the values the contract pins
DUPLEX_VECTORS = {("ACGT", "ACGT"): (4, 4), ("AAAAAAAA", "TTTTTTTT"): (8, 8), ("AAAAAAAA", "AAAAAAAA"): (0, 0), ("GGGGCCCC", "GGGGCCCC"): (8, 8),
                  ("CCCCCCCCCCCCCCCCCCAT", "CCCCCCCCCCCCCCCCCCAT"): (2, 2), ("CAGTCGATCGGATCCATGCA", "CAGTCGATCGGATCCATGCA"): (6, 4),
                  ("ACGTTGCAACGTACGTAGCT", "ACGTTGCAACGTACGTAGCT"): (12, 4), ("ACGTTGCAACGTACGTAGCT", "CAGTCGATCGGATCCATGCA"): (4, 4),
                  ("CAGTCGATCGGATCCATGCA", "ACGTTGCAACGTACGTAGCT"): (4, 4), ("GATTACAGATTACAGGC", "TTTGCCTGTAATC"): (10, 10),
                  ("GCGCGCGCGCGCGCGCGCGC", "GCGCGCGCGCGCGCGCGCGC"): (20, 20)}
HAIRPIN_VECTORS = {"GGGGCCCC": 2, "CAGTCGATCGGATCCATGCA": 3, "ACGTTGCAACGTACGTAGCT": 4, "GCGCGCGCGCGCGCGCGCGC": 8, "GGGGAAACCCC": 4, "GGGGAACCCC": 3, "GGGCTTTTGCCC": 4,
                   "GGGCTTTGCCC": 4, "GGGCTTGCCC": 3, "CCCCCAAAGGGGG": 5}


def pair_params(**fields):
    assert set(fields) <= set(PAIR_DEFAULTS)
    return dict(PAIR_DEFAULTS, **fields)


def reverse_complement(oligo: str) -> str:
    return "".join(COMPLEMENT[ch] for ch in reversed(oligo))


# ---- in letters
def duplex(a: str, b: str):
    """-> (any, end) of two oligos read 5' to 3'"""
    ka, kb = len(a), len(b)
    any_, end = 0, 0
    for c in range(ka + kb - 1):
        pairs = [i for i in range(ka) if 0 <= c - i < kb]      # consecutive i
        run = []
        for i in pairs + [None]:
            if i is not None and COMPLEMENT[a[i]] == b[c - i]:
                run.append(i)
                continue
            if run:
                any_ = max(any_, len(run))
                if ka - 1 in run or c - (kb - 1) in run:
                    end = max(end, len(run))
            run = []
    return any_, end


def hairpin(a: str) -> int:
    k, best = len(a), 0
    for c in range(2 * k - 1):
        run = 0
        for i in range(k):
            j = c - i
            if not 0 <= j < k:
                continue
            run = run + 1 if i < j and j - i - 1 >= HAIRPIN_LOOP and COMPLEMENT[a[i]] == a[j] else 0
            best = max(best, run)
    return best


def _i32(v: int) -> int:
    return v - (1 << 32) if v >= 1 << 31 else v


def _primer(letters: str, p: int, k: int, tm: int, penalty: int):
    bases = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(letters[p:p + k]))
    return (p, k, tm, penalty, _i32(bases & 0xffffffff), _i32(bases >> 32))


def side(letters: str, blocked, lo: int, hi: int, right: bool, prm, pair):
    """-> (the shortlist: (key, p, tm, oligo, self any, self end, hairpin) in order, admissible candidates, passing candidates)"""
    found, passing = 0, []
    for p in range(lo, hi):
        for k in range(prm["min_length"], prm["max_length"] + 1):
            if p + k > hi:
                break
            tm = admissible(letters, blocked, p, k, p if right else p + k - 1, prm)
            if tm is None:
                continue
            found += 1
            oligo = reverse_complement(letters[p:p + k]) if right else letters[p:p + k]
            (self_any, self_end), stem = duplex(oligo, oligo), hairpin(oligo)
            if self_any > pair["max_self_any"] or self_end > pair["max_self_end"] or stem > pair["max_hairpin"]:
                continue
            penalty = abs(tm - prm["tm_opt"]) + 10 * abs(k - prm["opt_length"])
            passing.append(((penalty, p - lo if right else hi - (p + k), k), p, tm, oligo, self_any, self_end, stem))
    passing.sort()
    return passing[:pair["shortlist"]], found, len(passing)


def choose(letters: str, left, right, counts, pair, duplex_of=duplex):
    """the record of one target from its two shortlists"""
    best, admissible_pairs = None, 0
    for l, a in enumerate(left):
        for r, b in enumerate(right):
            difference = abs(a[2] - b[2])
            if difference > pair["max_tm_difference"]:
                continue
            pair_any, pair_end = duplex_of(a[3], b[3])
            if pair_any > pair["max_pair_any"] or pair_end > pair["max_pair_end"]:
                continue
            admissible_pairs += 1
            key = (a[0][0] + b[0][0] + difference, b[1] + b[0][2] - a[1], l, r)
            if best is None or key < best[0]:
                best = (key, a, b, difference, pair_any, pair_end)
    tail = counts + (len(left) * len(right), admissible_pairs, 0)
    if best is None:
        return pc.NO_PRIMER * 2 + (0,) * 13 + tail
    key, a, b, difference, pair_any, pair_end = best
    return (_primer(letters, a[1], a[0][2], a[2], a[0][0]) + _primer(letters, b[1], b[0][2], b[2], b[0][0]) + (key[0], difference, key[1], key[2], key[3])
            + a[4:7] + b[4:7] + (pair_any, pair_end) + tail)


def record_primer_pairs(seq: bytes, rows, targets, prm=None, pair=None):
    """-> one tuple of the 32 values per target, in FIELDS' order"""
    prm, pair = prm or pc.DEFAULTS, pair or PAIR_DEFAULTS
    letters = seq.decode("latin-1").upper()
    blocked = blocked_positions(seq, rows)
    out = []
    for s, e in targets:
        s1, e1, lo, hi = clip(int(s), int(e), prm["flank"], len(seq))
        left, n_left, p_left = side(letters, blocked, lo, s1, False, prm, pair)
        right, n_right, p_right = side(letters, blocked, e1, hi, True, prm, pair)
        out.append(choose(letters, left, right, (n_left, n_right, p_left, p_right), pair))
    return out


# ---- the same with oligos as integers: base i at bits 2 i, A 0, C 1, G 2, T 3
EVEN = int("01" * 32, 2)


def pack(oligo: str) -> int:
    return sum("ACGT".index(ch) << (2 * i) for i, ch in enumerate(oligo))


def duplex_packed(a: str, b: str):
    ka, kb = len(a), len(b)
    x, y = pack(a), pack(b[::-1])      # y[i + d] = b[kb - 1 - d - i]: placement c = kb - 1 - d
    any_, end = 0, 0
    for d in range(-(ka - 1), kb):
        lo, hi = max(0, -d), min(ka, kb - d)
        z = x ^ (y >> (2 * d) if d >= 0 else y << (-2 * d))
        m = z & (z >> 1) & EVEN & ((1 << (2 * hi)) - 1) & ~((1 << (2 * lo)) - 1)
        if not m:
            continue
        t, run = m, 0
        while t:
            t &= t >> 2
            run += 1
        any_ = max(any_, run)
        if hi == ka:
            n = 0
            while n < ka - lo and (m >> (2 * (ka - 1 - n))) & 1:
                n += 1
            end = max(end, n)
        if d <= 0:
            n = 0
            while (m >> (2 * (lo + n))) & 1:
                n += 1
            end = max(end, n)
    return any_, end


class PairArrays(pc.RecordArrays):
    """RecordArrays, and for every length k and every admissible start whether the candidate passes the three self limits as a
    left oligo (its bases) and as a right oligo (their reverse complement): numpy words of 64 bits, one candidate each"""

    def __init__(self, seq: bytes, rows, prm, pair):
        super().__init__(seq, rows, prm)
        self.pair, L = pair, len(seq)
        table = np.zeros(256, dtype=np.uint64)
        for c, ch in enumerate("ACGT"):
            table[ord(ch)] = table[ord(ch.lower())] = c
        code = table[np.frombuffer(seq, np.uint8)]
        self.pass_left, self.pass_right = {}, {}
        for k in self.tm:
            for right, ok, out in ((False, self.left[k], self.pass_left), (True, self.right[k], self.pass_right)):
                at = np.flatnonzero(ok)
                o, rev = np.zeros(len(at), np.uint64), np.zeros(len(at), np.uint64)
                for j in range(k):      # oligo base j, and the oligo reversed
                    base = (np.uint64(3) - code[at + k - 1 - j]) if right else code[at + j]
                    o |= base << np.uint64(2 * j)
                    rev |= base << np.uint64(2 * (k - 1 - j))
                passes = np.zeros(L - k + 1, bool)
                passes[at] = self._within(o, rev, k)
                out[k] = passes

    @staticmethod
    def _has_run(m, n: int):
        """m holds n set even bits in a row"""
        if n > 32:
            return np.zeros(len(m), bool)
        for _ in range(n - 1):
            m = m & (m >> np.uint64(2))
        return m != 0

    def _within(self, o, rev, k: int):
        even, pair = np.uint64(EVEN), self.pair
        good = np.ones(len(o), bool)
        bases = lambda lo, hi: np.uint64(((1 << (2 * hi)) - 1) & ~((1 << (2 * lo)) - 1))
        for d in range(-(k - 1), k):
            lo, hi, c = max(0, -d), min(k, k - d), k - 1 - d
            z = o ^ (rev >> np.uint64(2 * d) if d >= 0 else rev << np.uint64(-2 * d))
            m = z & (z >> np.uint64(1)) & even & bases(lo, hi)
            good &= ~self._has_run(m, pair["max_self_any"] + 1)
            # a run through a 3' base is longer than T when the T + 1 pairs from that base on are all bonded
            t = pair["max_self_end"] + 1
            if hi - lo >= t:
                if hi == k:
                    good &= (m & bases(k - t, k)) != bases(k - t, k) & even
                if d <= 0:
                    good &= (m & bases(lo, lo + t)) != bases(lo, lo + t) & even
            top = (c - 1 - HAIRPIN_LOOP) // 2      # the last i with a loop of 3 between i and c - i
            if top >= lo:
                good &= ~self._has_run(m & bases(lo, min(top + 1, hi)), pair["max_hairpin"] + 1)
        return good

    def shortlist(self, lo: int, hi: int, right: bool):
        prm, found, passing = self.prm, 0, []
        for k, tm in self.tm.items():
            if lo + k > hi:
                continue
            found += int((self.right if right else self.left)[k][lo:hi - k + 1].sum())
            for p in (lo + np.flatnonzero((self.pass_right if right else self.pass_left)[k][lo:hi - k + 1])).tolist():
                t = int(tm[p])
                passing.append(((abs(t - prm["tm_opt"]) + 10 * abs(k - prm["opt_length"]), p - lo if right else hi - (p + k), k), p, t))
        passing.sort()
        out = []
        for key, p, t in passing[:self.pair["shortlist"]]:
            oligo = reverse_complement(self.letters[p:p + key[2]]) if right else self.letters[p:p + key[2]]
            out.append((key, p, t, oligo) + duplex_packed(oligo, oligo) + (hairpin(oligo),))
        return out, found, len(passing)


def record_primer_pairs_without_loops(seq: bytes, rows, targets, prm=None, pair=None):
    prm, pair = prm or pc.DEFAULTS, pair or PAIR_DEFAULTS
    arrays = PairArrays(seq, rows, prm, pair)
    out = []
    for s, e in np.asarray(targets, dtype=np.int64).reshape(-1, 2).tolist():
        s1, e1, lo, hi = clip(s, e, prm["flank"], len(seq))
        left, n_left, p_left = arrays.shortlist(lo, s1, False)
        right, n_right, p_right = arrays.shortlist(e1, hi, True)
        out.append(choose(arrays.letters, left, right, (n_left, n_right, p_left, p_right), pair, duplex_packed))
    return out


def as_tuples(arr):
    """a PRIMER_PAIRS_DT array as the tuples above"""
    return [tuple(int(v) for v in r) for r in arr.tolist()]


def primers_of(row):
    """the 14 values of primers_contract's FIELDS that a row of 32 holds: both primers and the two counts of candidates"""
    return tuple(row[:12]) + tuple(row[25:27])


# ---- the text
def pair_lines(bed: str, rows) -> str:
    lines = bed.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) == len(rows)
    out = []
    for line, r in zip(lines, rows):
        left, right = tuple(r[:6]), tuple(r[6:12])
        if left[0] >= 0 and right[0] >= 0:
            cols = [str(left[0]), str(left[0] + left[1]), pc.oligo_of(left), pc.tenths(left[2]),
                    str(right[0]), str(right[0] + right[1]), pc.oligo_of(right)[::-1].translate(pc.COMPLEMENT), pc.tenths(right[2]), str(r[14]), pc.tenths(r[13])]
            cols += [str(r[23]), str(r[24])] + [str(v) for v in r[17:23]]
        else:
            cols = ["."] * 18
        cols += [str(r[27]), str(r[28]), str(r[30])]
        out.append(line + "".join("\t" + c for c in cols) + "\n")
    return "".join(out)
