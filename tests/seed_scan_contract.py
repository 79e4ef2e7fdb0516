"""The seed scans between the dispatch list and the alignments, stated plainly from the reference text (line numbers cited),
and the constructed seed lists the tests of tests/test_seed_scans.py (CPU) and tests/test_seed_scans_gpu.py hand to the oracle,
the host twin and the device through `set_dispatch` / `adopt_dispatch`.

Pure Python and numpy.  Nothing here is derived from the kernels or from refine.cpp: where the two disagree, the reference
text decides.  Coordinates are sequence positions p = 0..L-1 (the reference stores p at bit L-1-p, fasta_utils.cpp:93).

Defined divergences shared with the oracle (undefined behaviour in the reference): positions from L on are never N (D3,
parse_smallmotif_seed.cpp:221-226 reads N_bset beyond the record there), and mostFrequentLongerMotif's seed end is clamped to L.
"""
import numpy as np

SEED_DT = np.dtype([("start", "<i4"), ("end", "<i4"), ("mlen", "<i4"), ("type", "<i4")])

_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _LUT[_c] = _i
    _LUT[_c + 32] = _i


_last_encoded = [None, None]


def encode(seq: bytes) -> np.ndarray:
    """one symbol per base: 0..3 = A C G T (either case), 4 = anything else (N_bset, fasta_utils.cpp:94-113)"""
    if _last_encoded[0] is not seq:             # (the functions below are called seed by seed over one record)
        sym = _LUT[np.frombuffer(bytes(seq), np.uint8)]
        sym.setflags(write=False)
        _last_encoded[:] = [seq, sym]
    return _last_encoded[1]


def default_params(m_lo: int, m_hi: int) -> dict:
    """MINIMUM_LENGTH / PERFECT_UNITS as ribbit.cpp:151-174 fills them, with the factor completion of :219-235; cones threshold 3
    (:191)"""
    min_length, known = {}, set()
    for k in range(m_lo, m_hi + 1):
        min_length[k] = max(12, 2 * k)
        known.add(k)
    units = {m: 8 if m == 1 else 4 if m == 2 else 3 if m == 3 else 2 for m in range(1, m_hi + 1)}
    for m in range(m_lo, m_hi + 1):
        for f in range(1, m // 2 + 1):
            if m % f == 0 and f not in known:
                min_length[f] = min_length[m]
                known.add(f)
    return {"min_length": min_length, "perfect_units": units, "threshold": 3}


def params_of(case) -> dict:
    """the thresholds a case runs with: the defaults of its handle, then the case's own"""
    p = default_params(case["m_lo"], case["m_hi"])
    spec = case.get("params", {})
    p["min_length"].update(spec.get("min_length", {}))
    p["perfect_units"].update(spec.get("perfect_units", {}))
    p["threshold"] = spec.get("threshold", p["threshold"])
    return p


def fill_params(rp, case):
    """the same thresholds in a RefineParams structure (the oracle's or the library's: one layout) that holds the defaults"""
    spec = case.get("params", {})
    for m, v in spec.get("min_length", {}).items():
        rp.min_length[m] = v
    for m, v in spec.get("perfect_units", {}).items():
        rp.perfect_units[m] = v
    if "threshold" in spec:
        rp.continuous_ones_threshold = spec["threshold"]
    return rp


# ------------------------------------------------------------------------------------------------ longestContinuousMatches
def longest_run(bits, start: int, end: int) -> int:
    """parse_seed.cpp:26-44 on bits[start:end] (one entry per base of the composed plane of the seed's motif length)"""
    l = best = 0
    for j in range(start, end):
        if bits[j] == 1:
            l += 1
        else:
            if l > best:
                best = l
            l = 0
    if l > best:
        best = l
    return best


def where_longest(bits, start: int, end: int) -> str:
    """in which 32-position word of the seed its (first) longest run of ones begins: "none", "only", "first", "last", "inside" """
    best, at, l = 0, -1, 0
    for j in range(start, end):
        l = l + 1 if bits[j] == 1 else 0
        if l > best:
            best, at = l, j - l + 1
    if best == 0:
        return "none"
    w0, w1 = start >> 5, (end - 1) >> 5
    if w0 == w1:
        return "only"
    return "first" if at >> 5 == w0 else "last" if at >> 5 == w1 else "inside"


# ------------------------------------------------------------------------------------------------------------ possibleMotifs
def warm_up(m: int) -> int:
    """the first j - seed_start with `j-seed_start >= (0.9*motif_length)-1` (parse_smallmotif_seed.cpp:104), in double arithmetic"""
    d = 0
    while not (d >= (0.9 * m) - 1):
        d += 1
    return d


def repeat_class(window: int, m: int) -> int:
    """calculateRepeatClass, bitseq_utils.cpp:185-221: the smallest of the m rotations of a 2m-bit word"""
    mask = (1 << (2 * m)) - 1
    best = window
    for i in range(m - 1):
        cycle = ((window >> (2 * (m - (i + 1)))) | (window << (2 * (i + 1)))) & mask
        if cycle < best:
            best = cycle
    return best


def seed_sequence_length(sym, start: int, end: int, m: int) -> int:
    """parse_smallmotif_seed.cpp:214-226 (= parse_seed.cpp:342-354): seed + one motif, cut at the first N below end + m"""
    length = (end - start) + m
    for s in range(start, end + m):
        if s < len(sym) and sym[s] == 4:
            length = s - start
            break
    return length


def small_motif_table(seq: bytes, start: int, end: int, m: int, min_len: int, min_units: int):
    """parse_smallmotif_seed.cpp:76-188 -> (early, classes): the reports pushed inside the loop (:120-129), in push order, as
    (class, MOTIF_START, MOTIF_END, MOTIF_UNITS); and every class the seed shows, in order of first appearance, as
    {"class", "first", "last", "units"} with its state when the loop ends (what :177-187 filters and reports)."""
    sym = encode(seq)
    L = len(sym)
    seed_end = start + seed_sequence_length(sym, start, end, m)
    if seed_end > L - 1:                                        # :94
        seed_end = L - 1
    mask = (1 << (2 * m)) - 1
    window = 0
    state = {}              # class -> [MOTIF_START, MOTIF_END, MOTIF_UNITS, new_motif_start]; a dict keeps first-appearance order
    early = []
    for j in range(start, seed_end):
        window |= int(sym[j]) & 3 if sym[j] < 4 else 0          # :99; N is 00 (fasta_utils.cpp:111-113)
        wstart, wend = j - (m - 1), j + 1
        if j - start >= (0.9 * m) - 1:                          # :104
            motif = repeat_class(window, m)
            st = state.get(motif)
            if st is None:                                      # :106-116
                state[motif] = [wstart, wend, 1, wstart]
            elif wstart - st[1] > 3 * m:                        # :120
                if st[1] - st[0] >= min_len and st[2] >= min_units:
                    early.append((motif, st[0], st[1], st[2]))
                st[:] = [wstart, wend, 1, wstart]               # :132-138
            else:
                if wstart - st[3] >= m:                         # :162-166
                    st[3] = wstart
                    st[2] += 1
                st[1] = wend                                    # :167
        window = (window << 2) & mask                           # :173
    classes = [{"class": k, "first": v[0], "last": v[1], "units": v[2]} for k, v in state.items()]
    return early, classes


def qualifies(c, min_len: int, min_units: int) -> bool:
    """:180 -- what is reported when the seed ends"""
    return c["last"] - c["first"] >= min_len and c["units"] >= min_units


def expected_head_and_records(seq: bytes, start: int, end: int, m: int, min_len: int, min_units: int, longest: int, threshold: int):
    """What include/ribbit_hip.h promises of ribbit_hip_small_motifs for one seed: (flags, early reports, classes, records).
    flags -1: no device result (m > 10, or the longest run is below the threshold, parse_smallmotif_seed.cpp:234-235);
    flags 1: a 65th class or a 65th early report occurs (records then unspecified: None); flags 0: records = the early reports,
    then all classes in order of first appearance if two or more qualify, else the one that does, or none."""
    if m > 10 or longest < threshold:
        return -1, None, None, None
    early, classes = small_motif_table(seq, start, end, m, min_len, min_units)
    if len(classes) > 64 or len(early) > 64:
        return 1, None, None, None
    passing = [c for c in classes if qualifies(c, min_len, min_units)]
    final = classes if len(passing) >= 2 else passing
    rec = [list(e) for e in early] + [[c["class"], c["first"], c["last"], c["units"]] for c in final]
    return 0, len(early), len(final), np.array(rec, dtype=np.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------- mostFrequentLongerMotif
def best_row(seq: bytes, start: int, ssl: int, m: int):
    """parse_seed.cpp:153-256, loops as they stand (the innermost `for i` of each diagonal counted with one numpy comparison)
    -> (mmotif_index, max_count, rows that reach max_count).  (*MATRIX[r])[c] == 1 <=> base c is A/C/G/T and equals base r
    (fasta_utils.cpp:94-113).  The first strict maximum wins (:240); with no positive count mmotif_index keeps its 0 (:169)."""
    sym = encode(seq)
    L = len(sym)
    seed_end = min(start + ssl, L)

    def ones(row0, col0, n):        # sum over i < n of MATRIX[row0+i][col0+i]
        if n <= 0:
            return 0
        c = sym[col0:col0 + n]
        return int(np.count_nonzero((c == sym[row0:row0 + n]) & (c < 4)))

    mmotif_index, max_count, ties = 0, 0, 0
    for row_start in range(start, seed_end - m + 1):            # :179
        row_count = 0
        d = row_start + m
        while d < seed_end:                                     # :184
            max_dindex, max_dcount = -2, 0
            for x in range(-2, 3):
                dcount = ones(row_start, d + x, min(m, seed_end - (d + x)))          # :189-192
                if dcount > max_dcount:
                    max_dcount, max_dindex = dcount, x
            row_count += max_dcount
            d += max_dindex
            d += m
        u = row_start - m
        while u > start:                                        # :203
            max_dindex, max_dcount = -2, 0
            for x in range(-2, 3):
                dcount = 0 if u + x < 0 else ones(row_start, u + x, m)                # :208-211 (the break can only hit i = 0)
                if dcount > max_dcount:
                    max_dcount, max_dindex = dcount, x
            row_count += max_dcount
            u += max_dindex
            u -= m
        if u < start and abs(u - start) < m:                    # :220
            last_row = row_start + m - 1
            pc = start + ((m + (u - start)) - 1)
            prefix_rows = m + (u - start)
            max_dcount = 0
            for x in range(-2, 3):
                dcount = 0
                for i in range(prefix_rows):                    # :229-233
                    c = pc + x - i
                    if c >= seed_end or c < start:
                        break
                    if sym[c] < 4 and sym[c] == sym[last_row - i]:
                        dcount += 1
                if dcount > max_dcount:
                    max_dcount = dcount
            row_count += max_dcount
        if row_count > max_count:                               # :240
            max_count, mmotif_index, ties = row_count, row_start, 1
        elif row_count == max_count and max_count > 0:
            ties += 1
    return mmotif_index, max_count, ties


def long_motif(seq: bytes, row: int, m: int):
    """parse_seed.cpp:246-253 + calculateAtomicityLongMotif (bitseq_utils.cpp:116-137) + calculateMotif (:14-38) in the reference's
    unchecked uint256_t (a unit longer than 128 bases loses its head) -> (atomicity, motif.substr(0, atomicity))"""
    sym = encode(seq)
    wrap = (1 << 256) - 1
    unit = 0
    for j in range(row, row + m):
        unit = ((unit << 2) | (int(sym[j]) & 3 if sym[j] < 4 else 0)) & wrap
    atom = m
    for f in range(1, m - m // 3):
        if (unit >> (2 * f)) == (((1 << (2 * (m - f))) - 1) & wrap & unit):
            atom = f
            break
    motif = "".join("ACGT"[(unit >> (2 * (m - 1 - i))) & 3] for i in range(m))
    return atom, motif[:atom]


# ---------------------------------------------------------------------------------------------------------------- generators
def rand(n: int, seed: int, alphabet: bytes = b"ACGT") -> bytes:
    rs = np.random.RandomState(seed)
    return bytes(np.frombuffer(alphabet, np.uint8)[rs.randint(0, len(alphabet), size=n)])


def aperiodic_unit(m: int, seed: int, alphabet: bytes = b"ACGT") -> bytes:
    """m bases none of whose proper rotations equals it (so a clean tandem repeat of it shows exactly m window contents)"""
    for k in range(1000):
        u = rand(m, seed * 1000 + k, alphabet)
        if all(u[r:] + u[:r] != u for r in range(1, m)):
            return u
    raise AssertionError("no aperiodic unit")


def substituted(block: bytes, every: int, seed: int) -> bytes:
    """the block with one base in `every` replaced by another one"""
    rs = np.random.RandomState(seed)
    b = bytearray(block)
    for p in range(every // 2, len(b), every):
        b[p] = [c for c in b"ACGT" if c != b[p]][rs.randint(3)]
    return bytes(b)


def seeds_of(rows) -> np.ndarray:
    a = np.zeros(len(rows), SEED_DT)
    for i, r in enumerate(rows):
        a[i] = tuple(r) if len(r) == 4 else tuple(r) + (5,)
    return a


WORD_EDGES = sorted(32 * k + d for k in range(4) for d in (0, 1, 31))


def longest_run_cases():
    """Seed lists for longestContinuousMatches: start and end at every pair of word edges {32k + 0, 1, 31}, start == end,
    one-word seeds, end == L, every motif length of the handle.  The planes are whatever the stages compose; the CPU test proves
    with the oracle's planes that whole-word runs over three words and more, and longest runs in the first, the last and an
    inner word of a seed, are among them."""
    pairs = [(s, e) for s in WORD_EDGES for e in WORD_EDGES if s <= e]
    L = 1000
    rows = [(s, e, m) for m in range(1, 13) for s, e in pairs]
    rows += [(s, L, m) for m in (1, 2, 7, 12) for s in (0, 1, 31, 32, 959, 960, 961, 991, 992, 999, 1000)]
    rows += [(s + 600, e + 600, m) for m in (1, 12) for s, e in pairs]
    cases = [{"name": "all_A_1000", "seq": b"A" * L, "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows)}]
    # a five-base repeat with single substitutions every 9 bases except in three clean stretches: in the first word of the
    # seeds below, across an inner word edge, and in the last word
    unit = b"ACGGT"
    body = bytearray(substituted(unit * 200, 9, 3))
    clean = unit * 200
    for a, b in ((3, 29), (150, 172), (355, 381)):
        body[a:b] = clean[a:b]
    seq = bytes(body)
    rows = []
    for m in (5, 10):
        rows += [(0, 128, m), (0, 96, m), (1, 127, m), (130, 200, m), (128, 256, m), (129, 255, m), (300, 384, m), (290, 383, m),
                 (320, 384, m), (0, 384, m), (31, 353, m), (0, 1000, m), (640, 1000, m)]
        rows += [(s, e, m) for s, e in pairs]
    rows += [(s + 128, e + 256, m) for m in range(2, 41) for s, e in pairs[::7]]
    cases.append({"name": "substituted_ACGGT", "seq": seq, "m_lo": 2, "m_hi": 40, "seeds": seeds_of(rows)})
    return cases


def _block_lengths(m: int):
    w = warm_up(m)
    lens = {0, 1, w - 1, w, w + 1, m, 2 * m}
    lens |= {t - m for t in (63, 64, 65, 127, 128, 129)}        # stop - start = end - start + m
    return sorted(x for x in lens if x >= 0)


def small_length_case():
    """every m in 1..10 over a clean and a substituted tandem repeat of that period; seed lengths around the warm-up and those
    that put stop - start at 63 .. 65 and 127 .. 129 (the kernel walks 64 positions a load)"""
    parts, rows, at = [rand(40, 100)], [], 40
    for m in range(1, 11):
        unit = aperiodic_unit(m, 110 + m)
        for kind in (0, 1):
            block = unit * (200 // m + 1)
            if kind:
                block = substituted(block, 2 * m + 3, 120 + m)
            for shift in (0, 1, 33):
                rows += [(at + shift, at + shift + n, m) for n in _block_lengths(m)]
            parts += [block, rand(20, 130 + m + kind)]
            at += len(block) + 20
    return {"name": "lengths", "seq": b"".join(parts), "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows), "params": {"threshold": 0}}


def small_n_case():
    """the first N at offset 0, 1, 63, 64, 65, len - 1, len, len + m - 1 from the seed's start (each cuts the sequence length), and
    one at end + m, which does not"""
    parts, rows, at = [rand(40, 200)], [], 40
    n = 100
    for m in (1, 3, 7, 10):
        unit = aperiodic_unit(m, 210 + m)
        for off in (0, 1, 63, 64, 65, n - 1, n, n + m - 1, n + m):
            block = bytearray(substituted(unit * (160 // m + 1), 31, 220 + off))
            block[10 + off] = ord("N")
            rows.append((at + 10, at + 10 + n, m))
            parts += [bytes(block), rand(12, 230 + off)]
            at += len(block) + 12
    case = {"name": "first_N", "seq": b"".join(parts), "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows), "params": {"threshold": 0}}
    sym = encode(case["seq"])
    cut = [seed_sequence_length(sym, int(s["start"]), int(s["end"]), int(s["mlen"])) for s in case["seeds"]]
    want = [min(off, n + m) for m in (1, 3, 7, 10) for off in (0, 1, 63, 64, 65, n - 1, n, n + m - 1, n + m)]
    assert cut == want, "an N is not where the case says"
    return case


def small_record_end_cases():
    """end in {L, L - 1, L - m, L - m - 1}: the walk stops at L - 1, the record's last base never enters a window"""
    cases = []
    for m in (1, 2, 5, 10):
        unit = aperiodic_unit(m, 300 + m)
        seq = rand(50, 310 + m) + substituted(unit * (150 // m + 1), 41, 320 + m)
        L = len(seq)
        rows = [(s, e, m) for s in (50, 61, L - 70) for e in (L, L - 1, L - m, L - m - 1)]
        cases.append({"name": f"record_end_m{m}", "seq": seq, "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows), "params": {"threshold": 0}})
    return cases


def _free_base_unit(m: int, seed: int):
    """an aperiodic unit over three bases, and the fourth"""
    spacer = b"ACGT"[seed % 4:seed % 4 + 1]
    return aperiodic_unit(m, seed, bytes(c for c in b"ACGT" if c != spacer[0])) if m > 1 else b"ACGT"[(seed + 1) % 4:(seed + 1) % 4 + 1], spacer


def class_run(m: int, n_classes: int, seed: int):
    """(bases, seed length): a stretch in which no base equals the base m before it, drawn again until a seed over it shows
    exactly n_classes rotation classes, one new class per window"""
    length = n_classes - m + warm_up(m)           # windows = (length + m) - warm
    for k in range(400):
        rs = np.random.RandomState(seed * 1000 + k)
        b = bytearray(rs.choice(list(b"ACGT"), m).astype(np.uint8).tobytes())
        while len(b) < length + m + 1:
            b.append([c for c in b"ACGT" if c != b[-m]][rs.randint(3)])
        bases = bytes(b)
        _, classes = small_motif_table(b"G" * 4 + bases + b"G" * 4, 4, 4 + length, m, 1, 1)
        if len(classes) == n_classes:
            return bases, length
    raise AssertionError("no draw with the wanted number of classes")


def small_limits_case():
    """min_length and perfect_units at 1 for every m: the 3m / 3m + 1 gap (one early report more), and 64 / 65 classes at
    m = 8, 9, 10 (64: every class qualifies, the whole table leaves the device; 65: flags 1)"""
    one = {m: 1 for m in range(1, 11)}
    prm = {"threshold": 0, "min_length": one, "perfect_units": dict(one)}
    parts, rows, at = [rand(40, 400)], [], 40
    checks = []
    for m in range(1, 11):
        unit, spacer = _free_base_unit(m, 410 + m)
        for g in (3 * m, 3 * m + 1):
            block = unit * 8 + spacer * g + unit * 8
            rows.append((at, at + len(block), m))
            checks.append(("gap", m, g, len(rows) - 1))
            parts += [block, spacer * (m + 2) + rand(20, 420 + m)]
            at += len(block) + m + 2 + 20
    for m in (8, 9, 10):
        for n_classes in (64, 65):
            bases, length = class_run(m, n_classes, 430 + m)
            rows.append((at, at + length, m))
            checks.append(("classes", m, n_classes, len(rows) - 1))
            parts += [bases, rand(20, 440 + m)]
            at += len(bases) + 20
    case = {"name": "limits", "seq": b"".join(parts), "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows), "params": prm, "checks": checks}
    seq = case["seq"]
    n_early = {}
    for kind, m, v, i in checks:
        s = case["seeds"][i]
        early, classes = small_motif_table(seq, int(s["start"]), int(s["end"]), m, 1, 1)
        if kind == "gap":
            n_early[(m, v)] = len(early)
        else:
            assert len(classes) == v, (m, v, len(classes))
            assert v != 64 or sum(qualifies(c, 1, 1) for c in classes) >= 2
    for m in range(1, 11):
        assert n_early[(m, 3 * m + 1)] == n_early[(m, 3 * m)] + 1, ("gap boundary", m, n_early[(m, 3 * m)], n_early[(m, 3 * m + 1)])
    return case


def early_report_record(K: int):
    """(record, seed): K blocks of six AC and nine T between G flanks, one seed over the blocks, m = 2: the AC class comes back
    K - 1 times more than 3m past its end, each time long enough to be reported"""
    seq = b"G" * 30 + (b"AC" * 6 + b"T" * 9) * K + b"G" * 30
    return seq, (30, 30 + 21 * K, 2)


def small_early_limit_cases():
    cases = []
    for K, n in ((65, 64), (66, 65)):
        seq, seed = early_report_record(K)
        p = default_params(1, 12)
        early, classes = small_motif_table(seq, seed[0], seed[1], 2, p["min_length"][2], p["perfect_units"][2])
        assert len(early) == n and len(classes) <= 64, (K, len(early), len(classes))
        assert sum(qualifies(c, p["min_length"][2], p["perfect_units"][2]) for c in classes) == 1
        cases.append({"name": f"early_reports_{n}", "seq": seq, "m_lo": 1, "m_hi": 12, "seeds": seeds_of([seed]), "params": {"threshold": 0},
                      "n_early": n})
    return cases


def small_layout_case():
    """one seed each with 0, 1, 2 and 5 classes that qualify at the seed's end (default thresholds, m = 3): the record layout of
    include/ribbit_hip.h; `survivors` names the counts, seed by seed"""
    reps = [b"ACG", b"TTG", b"CCA", b"GAT", b"CTA"]
    p = default_params(1, 12)
    none = next(b for b in (rand(40, 500 + k) for k in range(100))
                if not any(qualifies(c, p["min_length"][3], p["perfect_units"][3]) for c in small_motif_table(b"C" * 4 + b + b"C" * 8, 4, 44, 3, 12, 3)[1]))
    blocks = [none, b"ACG" * 12, b"ACG" * 10 + b"TTG" * 10, b"".join(r * 10 for r in reps)]
    parts, rows, at = [rand(30, 501)], [], 30
    for b in blocks:
        rows.append((at, at + len(b), 3))
        parts += [b, rand(25, 502 + len(rows), b"AC")]
        at += len(b) + 25
    case = {"name": "layout", "seq": b"".join(parts), "m_lo": 1, "m_hi": 12, "seeds": seeds_of(rows), "params": {"threshold": 0},
            "survivors": [0, 1, 2, 5]}
    for s, want in zip(case["seeds"], case["survivors"]):
        _, classes = small_motif_table(case["seq"], int(s["start"]), int(s["end"]), 3, p["min_length"][3], p["perfect_units"][3])
        assert sum(qualifies(c, p["min_length"][3], p["perfect_units"][3]) for c in classes) == want, want
    return case


def selection_case():
    """default threshold 3 over an all-A record (every composed plane is all ones there, so a seed's longest run is its length):
    a seed of two bases, one of three, and one with m = 11 -> no device result, a device result, no device result"""
    return {"name": "selection", "seq": b"A" * 400, "m_lo": 1, "m_hi": 12, "seeds": seeds_of([(100, 102, 3), (100, 103, 3), (100, 140, 11)]),
            "longest": [2, 3, 40], "flags": [-1, 0, -1]}


def arena_case():
    """200 copies of the layout case's seed with five survivors (ten records and more: every class leaves the device)"""
    base = small_layout_case()
    s = base["seeds"][3]
    p = default_params(1, 12)
    flags, n_early, n_cls, rec = expected_head_and_records(base["seq"], int(s["start"]), int(s["end"]), 3, p["min_length"][3], p["perfect_units"][3], 0, 0)
    assert flags == 0 and n_early + n_cls >= 10
    return {"name": "arena", "seq": base["seq"], "m_lo": 1, "m_hi": 12, "seeds": np.repeat(base["seeds"][3:4], 200), "params": {"threshold": 0},
            "records_per_seed": n_early + n_cls}


def small_table_cases():
    return ([small_length_case(), small_n_case()] + small_record_end_cases() + [small_limits_case()] + small_early_limit_cases()
            + [small_layout_case()])


LONG_M = (11, 12, 16, 31, 32, 33, 63, 64, 65, 100, 200)
LONG_ROWS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 500)


def _indel_copies(unit: bytes, copies: int, seed: int) -> bytes:
    """copies of the unit separated by indels of +-1 and +-2 bases (an inserted base, or the unit's tail dropped)"""
    rs = np.random.RandomState(seed)
    out = bytearray()
    for k in range(copies):
        d = (0, 1, -1, 2, -2)[k % 5]
        out += unit[:len(unit) + d] if d < 0 else unit + bytes(rs.choice(list(b"ACGT"), d).astype(np.uint8).tobytes())
    return bytes(out)


def _unrelated(m: int, n: int) -> bytes:
    """n < 2m bases in which no base equals a base m - 2 .. m + 2 further on: no diagonal of any row scores"""
    assert m >= 6 and n < 2 * m
    return (b"A" * (m - 2) + b"G" * 4 + b"C" * m)[:n]


def long_row_cases():
    """One record per motif length: for every row count of LONG_ROWS a seed whose sequence length is m + rows - 1 (an N behind it
    where the seed alone is shorter than 0.9 m asks), over an exact tandem repeat (every row ties), over copies separated by
    indels, and seeds of m <= ssl < 2m unrelated bases (no score: the motif is the record's first m bases, made distinctive).
    `expect` lists per seed what best_row must find: "tie", "zero" or None."""
    cases = []
    for m in LONG_M:
        head = rand(m, 600 + m)                                  # the record's first m bases, found nowhere else
        parts, rows, expect, at = [head, b"N"], [], [], m + 1
        unit = aperiodic_unit(m, 610 + m)
        for r in LONG_ROWS:
            for kind in ("tandem", "indel"):
                ssl = m + r - 1
                need = int(np.ceil(0.9 * m))
                seed_len = max(r - 1, need)                       # end - start
                with_n = seed_len + m > ssl                       # the N cuts the sequence length to ssl
                span = max(ssl, seed_len + m) + 3
                body = (unit * (span // m + 2)) if kind == "tandem" else _indel_copies(unit, span // m + 3, 620 + m + r)
                block = bytearray(body[:span])
                if with_n:
                    block[ssl] = ord("N")
                rows.append((at, at + seed_len, m))
                expect.append("tie" if kind == "tandem" and r >= 2 and ssl >= 2 * m else None)
                parts += [bytes(block), b"N"]
                at += span + 1
        for n in sorted({m, m + 1, m + m // 2, 2 * m - 1}):        # unrelated bases: zero score
            if m < 6:
                continue
            seed_len = max(int(np.ceil(0.9 * m)), n - m)
            block = _unrelated(m, n) + b"N" + rand(m, 630 + n, b"T")
            rows.append((at, at + seed_len, m))
            expect.append("zero")
            parts += [block, b"N"]
            at += len(block) + 1
        seq = b"".join(parts)
        case = {"name": f"rows_m{m}", "seq": seq, "m_lo": 2, "m_hi": 200, "seeds": seeds_of(rows), "params": {"threshold": 0}, "expect": expect}
        sym = encode(seq)
        got_rows = set()
        for s in case["seeds"][:2 * len(LONG_ROWS)]:
            ssl = seed_sequence_length(sym, int(s["start"]), int(s["end"]), m)
            got_rows.add(ssl - m + 1)
        assert got_rows == set(LONG_ROWS), (m, sorted(got_rows))
        cases.append(case)
    return cases


LAST_ROW_DRAWS = ((11, 65, 148), (16, 66, 7), (33, 65, 1376), (64, 129, 455))      # (m, rows, draw): found by search, checked below


def last_row_case():
    """seeds of random bases whose LAST row is the one strict maximum (rows = 65 and 129: that row is alone in its 64-row slice):
    a scan that loses the last row, or a slice, picks another window"""
    parts, rows, at = [rand(64, 690), b"N"], [], 65
    for m, r, k in LAST_ROW_DRAWS:
        ssl = m + r - 1
        body = rand(ssl, 900000 + 1000 * m + 7 * r + k * 131)
        rows.append((at, at + ssl - m, m))
        parts += [body, b"N"]
        at += ssl + 1
    case = {"name": "last_row", "seq": b"".join(parts), "m_lo": 2, "m_hi": 200, "seeds": seeds_of(rows), "params": {"threshold": 0},
            "expect": ["last"] * len(rows)}
    for s, (m, r, _) in zip(case["seeds"], LAST_ROW_DRAWS):
        row, score, ties = best_row(case["seq"], int(s["start"]), m + r - 1, m)
        assert (row, ties) == (int(s["start"]) + r - 1, 1) and score > 0, ("the last row no longer wins", m, r, row, score, ties)
    return case


def long_position_cases():
    """seeds that start at 0, 1 and 2 (the upstream walk meets columns below 0), seeds with end == L and with start + ssl > L, and
    an N directly behind a seed"""
    cases = []
    for m in (11, 32, 65):
        unit = aperiodic_unit(m, 700 + m)
        body = _indel_copies(unit, 6, 710 + m) + unit * 6
        seq = body + rand(40, 720 + m) + b"N" + unit * 5 + b"N" + rand(30, 730 + m) + substituted(unit * 7, 17, 740 + m)
        L = len(seq)
        n_at = len(body) + 40 + 1 + 5 * m                         # the N directly behind unit * 5
        rows = [(s, s + n, m) for s in (0, 1, 2) for n in (2 * m, 4 * m + 3, len(body) - 3)]
        rows += [(n_at - 5 * m, n_at, m), (n_at - 4 * m + 1, n_at, m)]
        rows += [(L - 6 * m, L, m), (L - 5 * m - 1, L - 1, m), (L - 3 * m, L - m + 1, m), (L - m, L, m), (L - m - 3, L - 2, m)]
        cases.append({"name": f"positions_m{m}", "seq": seq, "m_lo": 2, "m_hi": 200, "seeds": seeds_of(rows), "params": {"threshold": 0}})
        sym = encode(seq)
        assert sym[n_at] == 4 and seed_sequence_length(sym, n_at - 5 * m, n_at, m) == 5 * m
        assert any(int(s["start"]) + seed_sequence_length(sym, int(s["start"]), int(s["end"]), m) > L for s in cases[-1]["seeds"])
    return cases


def mixed_cases():
    """two mixed lists for the end-to-end comparison of the BED text: small and long motifs, every type rank, seeds in no
    particular order, overlapping and repeated, with the default thresholds (the planes decide which seeds are refined)"""
    cases = []
    for k, (m_lo, m_hi) in enumerate(((2, 40), (2, 200))):
        rs = np.random.RandomState(800 + k)
        parts, spans = [rand(60, 810 + k)], []
        at = 60
        for m in (2, 3, 5, 7, 10, 11, 16, 33, m_hi // 2, m_hi):
            unit = aperiodic_unit(m, 820 + m)
            for block in (unit * max(4, 90 // m), substituted(unit * max(5, 120 // m), 13, 830 + m), _indel_copies(unit, max(5, 100 // m), 840 + m)):
                spans.append((at, at + len(block), m))
                parts += [block, rand(int(rs.randint(5, 60)), 850 + len(spans)), b"N" * int(rs.randint(0, 2))]
                at += len(parts[-3]) + len(parts[-2]) + len(parts[-1])
        seq = b"".join(parts)
        L = len(seq)
        rows = []
        for a, b, m in spans:
            for _ in range(6):
                s = int(np.clip(a + rs.randint(-m, m + 1), 0, L))
                e = int(np.clip(b - m + rs.randint(-m, m + 1), s, L))
                mm = int(np.clip(m + (rs.randint(-1, 2) if rs.rand() < 0.3 else 0), m_lo, m_hi))
                rows.append((s, e, mm, int(rs.choice([5, 4, 3, 2, 1, 0]))))
        order = rs.permutation(len(rows))
        cases.append({"name": f"mixed_{m_lo}_{m_hi}", "seq": seq, "m_lo": m_lo, "m_hi": m_hi, "seeds": seeds_of([rows[i] for i in order])})
    return cases


def all_cases():
    return (longest_run_cases() + small_table_cases() + [selection_case(), arena_case()] + long_row_cases() + [last_row_case()] + long_position_cases()
            + mixed_cases())


def rejected_seeds(length: int, m_lo: int, m_hi: int):
    """seeds the scans cannot index (include/ribbit_hip.h, ribbit_hip_adopt_dispatch), each with what is wrong with it"""
    return [((-1, 10, m_lo, 5), "a negative start"), ((20, 19, m_lo, 5), "end < start"), ((0, length + 1, m_lo, 5), "end beyond the record"),
            ((length, length + 1, m_lo, 5), "end beyond the record"), ((0, 10, m_lo - 1, 5), "mlen below the range"),
            ((0, 10, m_hi + 1, 5), "mlen above the range")]


# ------------------------------------------------------------------------------------------------- shared by the two test modules
def oracle_params(case):
    import ctypes as C
    import oracle_lib
    rp = oracle_lib.RefineParams()
    oracle_lib.lib().rbo_refine_params_default(C.byref(rp), case["m_lo"], case["m_hi"])
    return fill_params(rp, case)


def library_params(case):
    import ctypes as C
    import ribbit_amd
    rp = ribbit_amd.RefineParams()
    ribbit_amd.load_library().ribbit_refine_params_default(C.byref(rp), case["m_lo"], case["m_hi"])
    return fill_params(rp, case)


JOB_FIELDS = ("seed_index", "seed_type", "motif_length", "atomicity", "query_start", "query_length", "ppr_length", "small")


def motifs_of(jobs, pool: bytes):
    return [pool[int(j["motif_offset"]):int(j["motif_offset"]) + int(j["atomicity"])].decode() for j in jobs]


def assert_same_jobs(got, want, what=""):
    """every field of every job and every motif string"""
    (gjobs, gpool), (wjobs, wpool) = got, want
    assert len(gjobs) == len(wjobs), (what, len(gjobs), len(wjobs))
    for f in JOB_FIELDS:
        bad = np.nonzero(gjobs[f] != wjobs[f])[0]
        assert len(bad) == 0, (what, f, int(bad[0]), gjobs[bad[0]], wjobs[bad[0]])
    assert motifs_of(gjobs, gpool) == motifs_of(wjobs, wpool), what


def assert_table_matches(case, head, rec, longest, seeds=None):
    """head / records of ribbit_hip_small_motifs against expected_head_and_records, seed by seed through head[i, 0] (the arena's
    order is arbitrary); -> the flags"""
    p = params_of(case)
    seeds = case["seeds"] if seeds is None else seeds
    assert len(head) == len(seeds)
    irec = rec.view("<i4").astype(np.int64).reshape(-1, 4)
    irec[:, 0] = rec[:, 0]                                   # the class is unsigned
    for i, s in enumerate(seeds):
        m = int(s["mlen"])
        flags, n_early, n_cls, want = expected_head_and_records(case["seq"], int(s["start"]), int(s["end"]), m, p["min_length"].get(m, 0),
                                                                p["perfect_units"].get(m, 0), int(longest[i]), p["threshold"])
        assert int(head[i, 3]) == flags, (case["name"], i, s, head[i], flags)
        if flags != 0:
            continue
        first = int(head[i, 0])
        assert (int(head[i, 1]), int(head[i, 2])) == (n_early, n_cls), (case["name"], i, s, head[i], n_early, n_cls)
        assert first >= 0 and first + n_early + n_cls <= len(irec), (case["name"], i, head[i], len(irec))
        got = irec[first:first + n_early + n_cls]
        assert np.array_equal(got, want), (case["name"], i, s, got.tolist(), want.tolist())
    return head[:, 3]


_CASES = {}


def cases_by_name():
    if not _CASES:
        _CASES.update((c["name"], c) for c in all_cases())
    return _CASES


_ORACLES = {}


def oracle_of(name):
    """(oracle with the case's list adopted, its (jobs, pool), the seeds' longest runs by longest_run on the oracle's planes, the
    planes by motif length): computed once per process and shared; nobody changes it"""
    if name not in _ORACLES:
        from oracle_lib import Oracle
        c = cases_by_name()[name]
        o = Oracle(c["seq"], c["m_lo"], c["m_hi"])
        o.run_all()
        o.set_dispatch(c["seeds"])
        assert np.array_equal(o.dispatch().view("<i4"), c["seeds"].view("<i4"))
        planes, longest = {}, []
        for s in c["seeds"]:
            m = int(s["mlen"])
            if m not in planes:
                planes[m] = o.plane(m)
            longest.append(longest_run(planes[m], int(s["start"]), int(s["end"])))
        _ORACLES[name] = (o, o.refine_jobs(oracle_params(c)), np.array(longest, dtype=np.int32), planes)
    return _ORACLES[name]


_BEST = {}


def best_rows_of(name):
    """per seed of a case what ribbit_hip_seed_best_rows must say: best_row's window start, or -1 for a seed that never reaches
    mostFrequentLongerMotif (m <= 10, shorter than 0.9 m: parse_seed.cpp:363, longest run below the threshold: :366-367); with
    best_row's (row, count, rows at that count) beside it.  Computed once per process."""
    if name not in _BEST:
        c = cases_by_name()[name]
        longest = oracle_of(name)[2]
        thr = params_of(c)["threshold"]
        sym = encode(c["seq"])
        rows, full = [], []
        for i, s in enumerate(c["seeds"]):
            start, end, m = int(s["start"]), int(s["end"]), int(s["mlen"])
            if m <= 10 or end - start < 0.9 * m or longest[i] < thr:
                rows.append(-1)
                full.append(None)
                continue
            full.append(best_row(c["seq"], start, seed_sequence_length(sym, start, end, m), m))
            rows.append(full[-1][0])
        _BEST[name] = (np.array(rows, dtype=np.int32), full)
    return _BEST[name]
