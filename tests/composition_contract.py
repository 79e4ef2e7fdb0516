"""The plain statement of the composition contract (include/ribbit_hip.h), written from the ASCII bytes alone: no bit planes, no
prefix of blocks.  A loop form that reads like the contract, a numpy-cumsum form for the large cases, the two text formatters,
and the row sets of the edge cases."""
import numpy as np

# the bases of a block of the GPU's prefix (composition.hip: COMP_BLOCK) -- the edge cases are laid around it
B = 256
FIELDS = ("a", "c", "g", "t", "other", "left", "left_gc", "left_other", "left_covered", "right", "right_gc", "right_other", "right_covered")
KINDS = "acgt"


def kind(byte: int) -> int:
    """0 .. 3 for A, C, G, T in either case, 4 for every other byte"""
    return KINDS.find(chr(byte | 0x20)) if chr(byte | 0x20) in KINDS else 4


def counts(seq: bytes, lo: int, hi: int):
    """[a, c, g, t, other] of seq[lo:hi]: the letters counted in either case, everything else is `other`"""
    piece = seq[lo:hi]
    out = [piece.count(ch.encode()) + piece.count(ch.upper().encode()) for ch in KINDS]
    return out + [len(piece) - sum(out)]


def clip(s, e, flank, length):
    s1 = min(max(s, 0), length)
    e1 = min(max(e, s1), length)
    return s1, e1, max(s1 - flank, 0), min(e1 + flank, length)


def covered_positions(length, rows):
    """which positions a non-empty row holds, clipped as the mask clips"""
    covered = np.zeros(length + 1, dtype=bool)
    for s, e in rows:
        s, e = max(int(s), 0), min(int(e), length)
        if s < e:
            covered[s:e] = True
    return covered[:length]


def record_composition(seq: bytes, rows, flank: int):
    """-> one tuple of the 13 values per row, in FIELDS' order"""
    length = len(seq)
    covered = covered_positions(length, rows)
    out = []
    for s, e in rows:
        s1, e1, lo, hi = clip(int(s), int(e), flank, length)
        row, left, right = counts(seq, s1, e1), counts(seq, lo, s1), counts(seq, e1, hi)
        out.append(tuple(row) + (s1 - lo, left[1] + left[2], left[4], int(covered[lo:s1].sum()))
                   + (hi - e1, right[1] + right[2], right[4], int(covered[e1:hi].sum())))
    return out


def record_base_windows(seq: bytes, window: int):
    """-> one tuple (a, c, g, t, other) per window"""
    return [tuple(counts(seq, k, min(k + window, len(seq)))) for k in range(0, len(seq), window)]


def kinds_of(seq: bytes) -> np.ndarray:
    """kind() of every byte"""
    table = np.full(256, 4, dtype=np.int64)
    for k, ch in enumerate(KINDS):
        table[ord(ch)] = table[ord(ch.upper())] = k
    return table[np.frombuffer(seq, dtype=np.uint8)]


def _prefixes(seq: bytes) -> np.ndarray:
    """(5, L + 1): prefix[k][p] = bytes of kind k before p"""
    kinds = kinds_of(seq)
    out = np.zeros((5, len(seq) + 1), dtype=np.int64)
    for k in range(5):
        np.cumsum(kinds == k, out=out[k, 1:])
    return out


def record_composition_without_loops(seq: bytes, rows, flank: int) -> np.ndarray:
    """the same as an (n, 13) int64 array, by cumulative sums"""
    length = len(seq)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    s = np.clip(rows[:, 0], 0, length)
    e = np.clip(np.maximum(rows[:, 1], s), None, length)
    lo, hi = np.maximum(s - flank, 0), np.minimum(e + flank, length)
    pre = _prefixes(seq)
    diff = np.zeros(length + 1, dtype=np.int64)
    ms, me = np.maximum(rows[:, 0], 0), np.minimum(rows[:, 1], length)
    some = ms < me
    np.add.at(diff, ms[some], 1)
    np.add.at(diff, me[some], -1)
    cov = np.concatenate([[0], np.cumsum(np.cumsum(diff)[:length] > 0)])
    between = lambda k, a, b: pre[k][b] - pre[k][a]
    cols = [between(k, s, e) for k in range(5)]
    for a, b in ((lo, s), (e, hi)):
        cols += [b - a, between(1, a, b) + between(2, a, b), between(4, a, b), cov[b] - cov[a]]
    return np.stack(cols, 1)


def record_base_windows_without_loops(seq: bytes, window: int) -> np.ndarray:
    """(ceil(L / W), 5) int64"""
    length = len(seq)
    edges = np.minimum(np.arange(0, length + window, window, dtype=np.int64), length)      # ceil(L / W) + 1 of them
    pre = _prefixes(seq)
    return np.stack([pre[k][edges[1:]] - pre[k][edges[:-1]] for k in range(5)], 1)


def as_tuples(arr):
    """a COMPOSITION_DT or BASE_COUNTS_DT array as the tuples above"""
    return [tuple(int(v) for v in r) for r in arr.tolist()]


def as_array(arr) -> np.ndarray:
    """... as an (n, 13) or (n, 5) int64 array"""
    return np.ascontiguousarray(arr).view("<i4").reshape(len(arr), -1).astype(np.int64)


# ---- the texts
def composition_lines(bed: str, rows) -> str:
    lines = bed.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    assert len(lines) == len(rows)
    return "".join(line + "".join(f"\t{v}" for v in r) + "\n" for line, r in zip(lines, rows))


def window_lines(name: str, length: int, window: int, windows) -> str:
    assert len(windows) == -(-length // window)
    return "".join(f"{name}\t{k * window}\t{min((k + 1) * window, length)}" + "".join(f"\t{v}" for v in w) + "\n" for k, w in enumerate(windows))


# ---- the edge cases
def edge_positions(length):
    return sorted({-3, 0, 1, 31, 32, 33, B - 1, B, B + 1, length - 1, length, length + 3})


def edge_case_sets(length):
    """named row sets: every pair (s, e) over the edge positions, reversed and empty pairs among them, all at once (they cover each
    other), the pairs at most a word long alone (they leave most positions uncovered), and a few sparse sets in which a flank
    meets another row or none"""
    at = edge_positions(length)
    pairs = [(s, e) for s in at for e in at]
    yield "every pair", pairs
    yield "the short pairs", [(s, e) for s, e in pairs if e - s <= 32]
    yield "no rows", []
    yield "one empty row", [(5, 5)]
    yield "two rows apart", [(1, 3), (length - 2, length)]
    yield "abutting rows", [(0, 32), (32, B), (B, B + 1)]
    yield "a row and a copy", [(31, 33), (31, 33), (B - 1, B + 1)]
    yield "the whole record and more", [(-3, length + 3), (0, length)]
    yield "out of range", [(-9, -3), (length, length + 3), (length + 3, length + 9), (2**31 - 1, -2**31), (-2**31, 2**31 - 1)]


ALPHABET = b"ACGTNacgtnRYx-"


def sequences(length, seed=0):
    """named records of `length` bytes: random bytes of ALPHABET, all N, one base throughout, a clean record whose last base alone
    is N, and a clean record with an N run across the first block edge"""
    clean = (b"ACGTTGCAAC" * (length // 10 + 1))[:length]
    run = clean[:B - 2] + b"N" * 4 + clean[B + 2:]
    yield "random", np.frombuffer(ALPHABET, np.uint8)[np.random.RandomState(seed).randint(0, len(ALPHABET), length)].tobytes()
    yield "all N", b"N" * length
    yield "one base", b"g" * length
    yield "a last N", clean[:-1] + b"N" * min(length, 1)
    yield "an N run over a block edge", run[:length]


def random_rows(length, rs, n, longest=300, reach=20):
    starts = rs.randint(-reach, length + reach + 1, n)
    return np.stack([starts, starts + rs.randint(-3, longest + 1, n)], 1).astype(np.int64)
