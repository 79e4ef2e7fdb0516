"""The plain statement of the primer contract (include/ribbit_hip.h), written from the ASCII bytes alone: no bit planes, no LDS, no
wave scans.  A loop form that reads like the contract (every candidate judged on its own letters), a numpy form for the large
cases (per-record arrays for every length, then a minimum per window), the text formatter, and the targets of the edge cases."""
import numpy as np

from composition_contract import clip, covered_positions

FIELDS = tuple(f"{side}_{n}" for side in ("left", "right") for n in ("start", "length", "tm", "penalty", "bases_lo", "bases_hi")) + ("left_candidates", "right_candidates")
DEFAULTS = dict(flank=200, min_length=18, max_length=25, opt_length=20, tm_min=570, tm_opt=600, tm_max=630, gc_min_percent=40, gc_max_percent=60, max_run=4, gc_clamp=1)
MAX_FLANK, MAX_LENGTH = 1000, 32
NO_PRIMER = (-1, 0, 0, 0, 0, 0)

# SantaLucia 1998: dH in 100 cal/mol, dS in 0.1 cal/(K mol), per step read 5' -> 3'
NN = {"AA": (-79, -222), "TT": (-79, -222), "AT": (-72, -204), "TA": (-72, -213), "CA": (-85, -227), "TG": (-85, -227), "GT": (-84, -224), "AC": (-84, -224),
      "CT": (-78, -210), "AG": (-78, -210), "GA": (-82, -222), "TC": (-82, -222), "CG": (-106, -272), "GC": (-98, -244), "GG": (-80, -199), "CC": (-80, -199)}
TERMINAL = {"A": (23, 41), "T": (23, 41), "C": (1, -28), "G": (1, -28)}
TM_VECTORS = {"GCGCGCGCGCGCGCGCGCGC": 771, "ATATATATATATATATATAT": 241, "ACGTTGCAACGTACGTAGCT": 546, "CAGTCGATCGGATCCATGCA": 541}


def params(**fields):
    assert set(fields) <= set(DEFAULTS)
    return dict(DEFAULTS, **fields)


def tm_of(oligo: str) -> int:
    """tenths of a degree Celsius of an oligo over ACGT of 2 bases or more"""
    k = len(oligo)
    h = sum(NN[oligo[j:j + 2]][0] for j in range(k - 1)) + TERMINAL[oligo[0]][0] + TERMINAL[oligo[-1]][0]
    s = sum(NN[oligo[j:j + 2]][1] for j in range(k - 1)) + TERMINAL[oligo[0]][1] + TERMINAL[oligo[-1]][1] - 11 * (k - 1) - 362
    assert h < 0 and s < 0
    return (10000 * -h) // -s - 2732


def blocked_positions(seq: bytes, rows) -> np.ndarray:
    """a position is blocked when its byte is none of ACGTacgt or a non-empty row, clipped as the mask clips, holds it"""
    other = ~np.isin(np.frombuffer(seq, np.uint8), np.frombuffer(b"ACGTacgt", np.uint8))
    return other | covered_positions(len(seq), rows)


def admissible(letters: str, blocked, p: int, k: int, three: int, prm):
    """-> the Tm of the candidate [p, p + k) whose 3' base is at `three`, or None when it is not admissible"""
    if blocked[p:p + k].any():
        return None
    oligo = letters[p:p + k]
    g = oligo.count("C") + oligo.count("G")
    if 100 * g < prm["gc_min_percent"] * k or 100 * g > prm["gc_max_percent"] * k:
        return None
    if prm["max_run"] < k and any(ch * (prm["max_run"] + 1) in oligo for ch in "ACGT"):
        return None
    if prm["gc_clamp"] and letters[three] not in "CG":
        return None
    tm = tm_of(oligo)
    return tm if prm["tm_min"] <= tm <= prm["tm_max"] else None


def _i32(v: int) -> int:
    return v - (1 << 32) if v >= 1 << 31 else v


def _primer(letters: str, p: int, k: int, tm: int, penalty: int):
    bases = sum("ACGT".index(ch) << (2 * j) for j, ch in enumerate(letters[p:p + k]))
    return (p, k, tm, penalty, _i32(bases & 0xffffffff), _i32(bases >> 32))


def side(letters: str, blocked, lo: int, hi: int, right: bool, prm):
    """the best admissible candidate of the window [lo, hi) and how many there are"""
    best, found = None, 0
    for p in range(lo, hi):
        for k in range(prm["min_length"], prm["max_length"] + 1):
            if p + k > hi:
                break
            tm = admissible(letters, blocked, p, k, p if right else p + k - 1, prm)
            if tm is None:
                continue
            found += 1
            penalty = abs(tm - prm["tm_opt"]) + 10 * abs(k - prm["opt_length"])
            key = (penalty, p - lo if right else hi - (p + k), k)
            if best is None or key < best[0]:
                best = (key, p, tm)
    if best is None:
        return NO_PRIMER, 0
    (penalty, _, k), p, tm = best
    return _primer(letters, p, k, tm, penalty), found


def record_primers(seq: bytes, rows, targets, prm=None):
    """-> one tuple of the 14 values per target, in FIELDS' order"""
    prm = prm or DEFAULTS
    letters = seq.decode("latin-1").upper()
    blocked = blocked_positions(seq, rows)
    out = []
    for s, e in targets:
        s1, e1, lo, hi = clip(int(s), int(e), prm["flank"], len(seq))
        left, n_left = side(letters, blocked, lo, s1, False, prm)
        right, n_right = side(letters, blocked, e1, hi, True, prm)
        out.append(left + right + (n_left, n_right))
    return out


# ---- the same by arrays
class RecordArrays:
    """for every length k the Tm of every start of the record and whether the candidate there is admissible as a left and as a
    right one: what the targets' windows are cut from"""

    def __init__(self, seq: bytes, rows, prm):
        self.prm, self.letters, L = prm, seq.decode("latin-1").upper(), len(seq)
        table = np.full(256, 4, dtype=np.int64)
        for c, ch in enumerate("ACGT"):
            table[ord(ch)] = table[ord(ch.lower())] = c
        code = table[np.frombuffer(seq, np.uint8)]
        pre = lambda flags: np.concatenate([[0], np.cumsum(flags)]).astype(np.int64)
        blocked, gc = pre(blocked_positions(seq, rows)), pre((code == 1) | (code == 2))
        # the run of equal bytes that ends at i
        heads = np.flatnonzero(np.concatenate([[True], code[1:] != code[:-1]])) if L else np.zeros(0, np.int64)
        run = np.arange(L) - np.repeat(heads, np.diff(np.concatenate([heads, [L]]))) + 1 if L else np.zeros(0, np.int64)
        long_run = pre(run > prm["max_run"])
        nn_h, nn_s = np.zeros((5, 5), np.int64), np.zeros((5, 5), np.int64)
        for pair, (dh, ds) in NN.items():
            nn_h["ACGT".index(pair[0]), "ACGT".index(pair[1])], nn_s["ACGT".index(pair[0]), "ACGT".index(pair[1])] = dh, ds
        step_h, step_s = pre(nn_h[code[:-1], code[1:]]), pre(nn_s[code[:-1], code[1:]])      # step j: positions j, j + 1
        is_gc = (code == 1) | (code == 2)
        term_h, term_s = np.where(is_gc, 1, 23), np.where(is_gc, -28, 41)
        self.tm, self.left, self.right = {}, {}, {}
        for k in range(prm["min_length"], prm["max_length"] + 1):
            n = L - k + 1
            if n <= 0:
                continue
            p = np.arange(n)
            ok = blocked[p + k] == blocked[p]
            g = gc[p + k] - gc[p]
            ok &= (100 * g >= prm["gc_min_percent"] * k) & (100 * g <= prm["gc_max_percent"] * k)
            if k > prm["max_run"]:      # a run of max_run + 1 inside [p, p + k) ends at one of p + max_run .. p + k - 1
                ok &= long_run[p + k] == long_run[p + prm["max_run"]]
            h = step_h[p + k - 1] - step_h[p] + term_h[p] + term_h[p + k - 1]
            s = step_s[p + k - 1] - step_s[p] + term_s[p] + term_s[p + k - 1] - 11 * (k - 1) - 362
            tm = np.where(ok, (10000 * -h) // np.where(ok, -s, 1) - 2732, 0)
            ok &= (tm >= prm["tm_min"]) & (tm <= prm["tm_max"])
            clamp = is_gc if prm["gc_clamp"] else np.ones(L, bool)
            self.tm[k], self.left[k], self.right[k] = tm, ok & clamp[p + k - 1], ok & clamp[p]

    def side(self, lo: int, hi: int, right: bool):
        prm, best, found = self.prm, None, 0
        for k, tm in self.tm.items():
            if lo + k > hi:
                continue
            p = lo + np.flatnonzero((self.right if right else self.left)[k][lo:hi - k + 1])
            if not len(p):
                continue
            found += len(p)
            penalty = np.abs(tm[p] - prm["tm_opt"]) + 10 * abs(k - prm["opt_length"])
            distance = p - lo if right else hi - (p + k)
            key = (penalty << 32) | (distance << 8) | k
            j = int(key.argmin())
            if best is None or int(key[j]) < best[0]:
                best = (int(key[j]), int(p[j]), k, int(tm[p[j]]), int(penalty[j]))
        return (NO_PRIMER if best is None else _primer(self.letters, *best[1:])), found


def record_primers_without_loops(seq: bytes, rows, targets, prm=None):
    prm = prm or DEFAULTS
    arrays = RecordArrays(seq, rows, prm)
    out = []
    for s, e in np.asarray(targets, dtype=np.int64).reshape(-1, 2).tolist():
        s1, e1, lo, hi = clip(s, e, prm["flank"], len(seq))
        left, n_left = arrays.side(lo, s1, False)
        right, n_right = arrays.side(e1, hi, True)
        out.append(left + right + (n_left, n_right))
    return out


def as_tuples(arr):
    """a PRIMERS_DT array as the tuples above"""
    return [tuple(int(v) for v in r) for r in arr.tolist()]


# ---- the text
COMPLEMENT = str.maketrans("ACGT", "TGCA")


def oligo_of(primer) -> str:
    """the forward-strand bases of (start, length, tm, penalty, bases_lo, bases_hi)"""
    bases = (primer[5] & 0xffffffff) << 32 | (primer[4] & 0xffffffff)
    return "".join("ACGT"[(bases >> (2 * j)) & 3] for j in range(primer[1]))


def tenths(tm: int) -> str:
    return f"{'-' if tm < 0 else ''}{abs(tm) // 10}.{abs(tm) % 10}"


def primer_lines(bed: str, rows) -> str:
    lines = bed.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) == len(rows)
    out = []
    for line, r in zip(lines, rows):
        left, right = tuple(r[:6]), tuple(r[6:12])
        cols = [str(left[0]), str(left[0] + left[1]), oligo_of(left), tenths(left[2])] if left[0] >= 0 else ["."] * 4
        cols += [str(right[0]), str(right[0] + right[1]), oligo_of(right)[::-1].translate(COMPLEMENT), tenths(right[2])] if right[0] >= 0 else ["."] * 4
        cols += [str(right[0] + right[1] - left[0]) if left[0] >= 0 and right[0] >= 0 else ".", str(r[12]), str(r[13])]
        out.append(line + "".join("\t" + c for c in cols) + "\n")
    return "".join(out)


# ---- the cases
ALPHABET = b"ACGTNacgtnRYx-"


def random_record(length: int, seed=0, alphabet=ALPHABET) -> bytes:
    return np.frombuffer(alphabet, np.uint8)[np.random.RandomState(seed).randint(0, len(alphabet), length)].tobytes()


def clean_record(length: int, seed=0) -> bytes:
    """letters only, upper and lower case: most windows hold admissible candidates"""
    return random_record(length, seed, b"ACGTacgt")


def edge_targets(length: int):
    """targets whose windows start or end at the record's ends and at word edges, reversed, empty and out of range"""
    at = sorted({-3, 0, 1, 31, 32, 33, 63, 64, 65, length // 2, length - 33, length - 32, length - 1, length, length + 3})
    return [(s, e) for s in at for e in at if e - s in (-2, 0, 1, 7) or (s, e) in ((at[0], at[-1]), (at[1], at[-2]))] + [(2**31 - 1, -2**31), (-2**31, 2**31 - 1)]


def random_targets(length: int, rs, n: int, longest=60, reach=20):
    starts = rs.randint(-reach, length + reach + 1, n)
    return np.stack([starts, starts + rs.randint(-3, longest + 1, n)], 1).astype(np.int64)
