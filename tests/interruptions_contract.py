"""The decode of the rows' CIGARs as include/ribbit_hip.h states it, in plain Python: a regular expression for the grammar and loops
for the rest.  Shared by test_interruptions.py (host twin) and test_interruptions_gpu.py (device): both must equal this, and
check_properties() asserts what follows from the contract on any result."""
import re

import numpy as np

OP = re.compile(rb"([0-9]{1,10})([=MXID])")
INT32_MAX = (1 << 31) - 1
SITE_FIELDS = ("row", "start", "end", "x", "ins", "del", "cigar_at", "cigar_len")
ROW_FIELDS = ("first", "count", "x", "ins", "del", "query", "pure_start", "pure_end")


class BadCigar(ValueError):
    """.args = (row, byte offset within the pool or None)"""


def ops_of(cigar: bytes, row=0, base=0):
    """[(length, letter, offset of the first digit, offset behind the letter)], offsets counted from `base`"""
    ops, at = [], 0
    while at < len(cigar):
        m = OP.match(cigar, at)
        if not m or not 1 <= int(m.group(1)) <= INT32_MAX:
            raise BadCigar(row, base + at)
        ops.append((int(m.group(1)), m.group(2), base + at, base + m.end()))
        at = m.end()
    return ops


def record_interruptions(sequence: bytes, intervals, cigars):
    """-> (rows as tuples in ROW_FIELDS order, sites as tuples in SITE_FIELDS order, the observed bases per site)"""
    L = len(sequence)
    rows, sites, observed, base = [], [], [], 0
    for i, ((s, e), cigar) in enumerate(zip(intervals, cigars)):
        s, cigar = int(s), bytes(cigar)
        ops = ops_of(cigar, i, base)
        if sum(o[0] for o in ops) > INT32_MAX:
            raise BadCigar(i, None)
        q, first = 0, len(sites)
        stretches, mine = [], []          # [from, to) in q; [q from, q to, x, ins, del, cigar from, cigar to]
        before = None
        for length, letter, at, behind in ops:
            match = letter in b"=M"
            step = 0 if letter == b"D" else length
            if match:
                if before is True:
                    stretches[-1][1] = q + step
                else:
                    stretches.append([q, q + step])
            else:
                if before is not False:
                    mine.append([q, q, 0, 0, 0, at, behind])
                k = mine[-1]
                k[1] = q + step
                k[2 + b"XID".index(letter)] += length
                k[6] = behind
            q += step
            before = match
        if s + q > INT32_MAX:
            raise BadCigar(i, None)
        pure = (s, s)
        best = 0
        for a, b in stretches:
            if b - a > best:              # (strictly: the leftmost among equals stays)
                best, pure = b - a, (s + a, s + b)
        for k in mine:
            sites.append((i, s + k[0], s + k[1], k[2], k[3], k[4], k[5], k[6] - k[5]))
            a = min(max(s + k[0], 0), L)
            b = min(max(s + k[1], a), L)
            observed.append(sequence[a:b])
        rows.append((first, len(mine), sum(k[2] for k in mine), sum(k[3] for k in mine), sum(k[4] for k in mine), q, pure[0], pure[1]))
        base += len(cigar)
    return rows, sites, observed


def unpack(rows, sites, observed, offsets):
    """the library's result (numpy records, bytes, offsets) in the contract's form"""
    assert len(offsets) == len(sites) + 1 and int(offsets[0]) == 0 and len(observed) == int(offsets[-1])
    return ([tuple(int(r[f]) for f in ROW_FIELDS) for r in rows], [tuple(int(k[f]) for f in SITE_FIELDS) for k in sites],
            [observed[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])])


def check_properties(sequence, intervals, cigars, rows, sites, observed):
    """what follows from the contract, asserted on a result in the contract's form"""
    pool = b"".join(bytes(c) for c in cigars)
    assert len(rows) == len(intervals) == len(cigars)
    assert sum(r[1] for r in rows) == len(sites) == len(observed)
    at = 0
    start_of = np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).astype(int)
    for i, ((s, e), r) in enumerate(zip(intervals, rows)):
        s = int(s)
        first, count, x, ins, dele, query, pure_start, pure_end = r
        assert first == at                                               # the prefix sum
        mine = sites[first:first + count]
        at += count
        assert (x, ins, dele) == tuple(sum(k[f] for k in mine) for f in (3, 4, 5))
        ops = ops_of(bytes(cigars[i]))
        assert query == sum(n for n, c, _, _ in ops if c != b"D")
        # stretches and interruptions alternate and tile [s, s + query)
        matches = [(n, c) for n, c, _, _ in ops if c in b"=M"]
        pieces, q = [], 0                                                # ("stretch" | "site", from, to) rebuilt from the ops
        for n, c, _, _ in ops:
            kind = "stretch" if c in b"=M" else "site"
            step = 0 if c == b"D" else n
            if pieces and pieces[-1][0] == kind:
                pieces[-1][2] += step
            else:
                pieces.append([kind, s + q, s + q + step])
            q += step
        assert [p[0] for p in pieces] == [("stretch", "site")[(k + (pieces[0][0] == "site")) % 2] for k in range(len(pieces))] if pieces else True
        assert all(a[2] == b[1] for a, b in zip(pieces, pieces[1:]))
        assert not pieces or (pieces[0][1] == s and pieces[-1][2] == s + query)
        assert [(p[1], p[2]) for p in pieces if p[0] == "site"] == [(k[1], k[2]) for k in mine]
        stretches = [(p[1], p[2]) for p in pieces if p[0] == "stretch"]
        if stretches:
            longest = max(b - a for a, b in stretches)
            assert (pure_start, pure_end) == next((a, b) for a, b in stretches if b - a == longest)
            assert sum(n for n, _ in matches) == sum(b - a for a, b in stretches)
        else:
            assert (pure_start, pure_end) == (s, s)
        rebuilt, behind = b"", int(start_of[i])
        for k in mine:
            assert k[0] == i and s <= k[1] <= k[2] <= s + query        # every interruption lies in [s, s + query]
            assert k[3] + k[4] == k[2] - k[1]                            # x + ins == end - start
            assert k[3] + k[4] + k[5] > 0 and k[6] >= behind and k[7] >= 2
            between = pool[behind:k[6]]                                  # the match ops between two interruptions
            assert all(c in b"=M" for _, c, _, _ in ops_of(between)) and (between or behind == start_of[i])
            rebuilt += between + pool[k[6]:k[6] + k[7]]
            assert all(c in b"XID" for _, c, _, _ in ops_of(pool[k[6]:k[6] + k[7]]))
            behind = k[6] + k[7]
        tail = pool[behind:int(start_of[i + 1])]
        assert all(c in b"=M" for _, c, _, _ in ops_of(tail))
        assert rebuilt + tail == bytes(cigars[i])                        # the slices, joined with the match ops, rebuild the CIGAR
    L = len(sequence)
    for k, text in zip(sites, observed):
        a = min(max(k[1], 0), L)
        assert text == sequence[a:min(max(k[2], a), L)]


def random_cigar(rs, ops, kinds=b"=XIDM=="):
    """a CIGAR of `ops` ops with lengths skewed to the short"""
    out = b""
    for _ in range(ops):
        n = int(rs.choice([1, 1, 2, 3, 5, 12, 82, 300]))
        out += b"%d%c" % (n, kinds[rs.randint(len(kinds))])
    return out


def query_of(cigar):
    return sum(n for n, c, _, _ in ops_of(bytes(cigar)) if c != b"D")


SHAPES = [b"", b"5=", b"2X5=", b"5=1I", b"2X1I3D", b"3=2M4=", b"4=1X4=1D2=", b"3=1X3=1X2=", b"2=3D2=", b"2147483647=", b"0000000005=1X",
          b"1D", b"1M1X1M", b"7M", b"3=1X3=1X5=1D82="]


def edge_case_sets(L):
    """[(intervals, motif lengths, cigars)]: every CIGAR shape of the contract, rows that start before 0, end past L and lie wholly
    outside the record, consistent and not"""
    sets = []
    starts = [0, 1, L // 2, max(L - 3, 0), L, -4, L + 7]
    iv, ks, cg = [], [], []
    for j, shape in enumerate(SHAPES):
        for t, s in enumerate(starts):
            if shape == b"2147483647=" and s > 0:
                continue                                                  # (s + query must fit int32)
            q = query_of(shape)
            iv.append((s, s + q if (j + t) % 5 else s + q + 1))           # every fifth row is inconsistent
            ks.append(1 + (j + t) % 4)
            cg.append(shape)
    sets.append((np.array(iv, dtype=np.int64), np.array(ks), cg))
    sets.append((np.array([(2, 9)], dtype=np.int64), np.array([2]), [b"3=1X3="]))
    sets.append((np.array([(-3, 2), (L - 2, L + 3), (L + 1, L + 6), (-9, -4)], dtype=np.int64), np.array([1, 2, 3, 4]), [b"1X3=1I"] * 4))
    sets.append((np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.int64), []))
    sets.append((np.array([(0, 0), (1, 1), (2, 2)], dtype=np.int64), np.array([1, 1, 1]), [b"", b"", b""]))
    return sets


def random_record(rs, t):
    """(sequence, intervals, motif lengths, cigars): records of a few dozen rows, some with many ops, some inconsistent"""
    L = int(rs.choice([0, 1, 64, 300, 4100, 20_000]))
    sequence = np.frombuffer(b"ACGTNacgtn", np.uint8)[rs.randint(0, 10, L)].tobytes()
    n = int(rs.randint(1, 70))
    iv, ks, cg = [], [], []
    for i in range(n):
        ops = int(rs.choice([0, 1, 1, 2, 3, 5, 8, 8, 40])) if (t + i) % 17 else 400
        c = random_cigar(rs, ops)
        s = int(rs.randint(-20, L + 20))
        iv.append((s, s + query_of(c) + (0 if rs.randint(6) else int(rs.randint(1, 4)))))
        ks.append(int(rs.randint(1, 9)))
        cg.append(c)
    return sequence, np.array(iv, dtype=np.int64), np.array(ks), cg


def cigar_of_bytes(rs, nbytes):
    """a valid CIGAR of exactly `nbytes` bytes (0, or 2 and more): ops of two or three bytes, kinds mixed"""
    assert nbytes == 0 or nbytes >= 2
    out = b""
    while len(out) < nbytes:
        left = nbytes - len(out)
        size = 3 if left == 3 or (left >= 5 and rs.randint(2)) else 2
        out += b"%d%c" % (rs.randint(10, 100) if size == 3 else rs.randint(1, 10), b"=X=I=DM"[rs.randint(7)])
    return out


def rebuilt_cigar(pool, start, end, mine):
    """the CIGAR pool[start:end] put together again from the interruptions' slices and the match ops between them"""
    out, behind = b"", start
    for k in mine:
        between = pool[behind:k[6]]
        assert all(c in b"=M" for _, c, _, _ in ops_of(between))
        out += between + pool[k[6]:k[6] + k[7]]
        behind = k[6] + k[7]
    assert all(c in b"=M" for _, c, _, _ in ops_of(pool[behind:end]))
    return out + pool[behind:end]
