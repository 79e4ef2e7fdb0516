"""The pairing of a scan's START / END events into run records, stated plainly (include/ribbit_hip.h, "Perfect stage of one chunk"
and ribbit_hip_scan_perfect_chunk), and the constructed, sharded event streams that tests/test_pairing_contract.py
(CPU) and tests/test_pairing_sharded_gpu.py hand to the host pairing and to the pairing kernels.

Plain Python: sequential walks over lists of (pos, mlen, kind) tuples; numpy only carries the words to the library and back.
Nothing here is derived from the kernels.

An event is pos | mlen << 32 | kind << 48 with kind 0 START, 1 / 2 / 3 END (mismatch / N / end of sequence); a run record is
(start, end, mlen, term) with term = kind - 1.  A scan leaves its events in SHARDS regions of region_cap words; the events of one
(motif, tile) -- tile = pos // TILE, ntile = length // TILE + 1 -- form one chunk, in position order, contiguous in one region;
a region's counter says how many words the scan wanted to write there, which may be more than region_cap.
"""
import functools
import random

import numpy as np

TILE = 16384
SHARDS = 64
S, E0, EN, EE = 0, 1, 2, 3
NOT_OWNED, HALF_START, HALF_END = -1, 3, 4                      # RIBBIT_RUN_* of include/ribbit_hip.h
BAD_EVENT, DUP_CHUNK, NOT_ALTERNATING, UNTERMINATED, NO_ROOM = 1, 2, 4, 8, 16      # PAIR_* of device_planes.h
RUN_DT = np.dtype([("start", "<i4"), ("end", "<i4"), ("mlen", "<i4"), ("term", "<i4")])
WHOLE = (0, 2 ** 63 - 1, 0)                                    # own_lo, own_hi, pos_offset of a whole record
FILLER = (7, 0xFFFF, 5)                                         # what unused slots hold: no launch has this motif, no event this kind


def pack(pos, mlen, kind):
    return pos | (mlen << 32) | (kind << 48)


def unpack(word):
    word = int(word)
    return word & 0xFFFFFFFF, (word >> 32) & 0xFFFF, (word >> 48) & 0xF


def ntile_of(length):
    return length // TILE + 1


# ------------------------------------------------------------------------------------------------------------------ the pairing
def pair(events, m_lo, nm, length, own_lo, own_hi, pos_offset):
    """events: (pos, mlen, kind) in (motif, position) order.  -> (slots, halves): one slot per START in (motif, start) order, and the
    halves of the runs the own range [own_lo, own_hi) cuts.  A slot is the whole run, positions shifted by pos_offset, when its START is
    owned and its END lies before own_hi; otherwise a place holder (0, 0, 0, NOT_OWNED) and at most one half: (start, -1, mlen,
    HALF_START) when the START is owned, else (-1, end, mlen, HALF_END + term) when the END is owned, else none.
    A stream that is not well formed raises ValueError."""
    slots, halves = [], []
    at = 0
    for mlen in range(m_lo, m_lo + nm):
        last = -1
        while at < len(events) and events[at][1] == mlen:
            pos, _, kind = events[at]
            if kind != S:
                raise ValueError(f"motif {mlen}: END at {pos} with no run open")
            if at + 1 == len(events) or events[at + 1][1] != mlen:
                raise ValueError(f"motif {mlen}: the run from {pos} never ends")
            end, _, end_kind = events[at + 1]
            if end_kind not in (E0, EN, EE) or not last < pos < end <= length:
                raise ValueError(f"motif {mlen}: START {pos} is followed by kind {end_kind} at {end} (record of {length})")
            term = end_kind - 1
            start_owned = own_lo <= pos < own_hi
            end_owned = own_lo <= end < own_hi
            if start_owned and end < own_hi:
                slots.append((pos + pos_offset, end + pos_offset, mlen, term))
            else:
                slots.append((0, 0, 0, NOT_OWNED))
                if start_owned:
                    halves.append((pos + pos_offset, -1, mlen, HALF_START))
                elif end_owned:
                    halves.append((-1, end + pos_offset, mlen, HALF_END + term))
            last = end
            at += 2
    if at != len(events):
        raise ValueError(f"event {at} {events[at]} is out of (motif, position) order or outside motifs {m_lo}..{m_lo + nm - 1}")
    return slots, halves


def events_of(truth_runs):
    """the events of a list of true runs (start, end, mlen, term), in (motif, position) order"""
    out = []
    for start, end, mlen, term in truth_runs:
        out.append((start, mlen, S))
        out.append((end, mlen, term + 1))
    out.sort(key=lambda e: (e[1], e[0]))
    return out


def chunks_of(events):
    """events in (motif, position) order cut into the chunks a scan makes of them: [(mlen, tile, [events])] in (motif, tile) order"""
    chunks = []
    for e in events:
        key = (e[1], e[0] // TILE)
        if not chunks or (chunks[-1][0], chunks[-1][1]) != key:
            chunks.append((key[0], key[1], []))
        chunks[-1][2].append(e)
    return chunks


# ------------------------------------------------------------------------------------------------------------- placing the events
def place(chunks, deal, region_cap):
    """chunks: [(mlen, tile, [events])]; deal(k, mlen, tile, n) -> (shard, slot) of chunk k's first event.  -> (event array of SHARDS *
    region_cap words, SHARDS counters).  Every chunk lands whole; the used slots of a region must be slots 0 .. counter - 1 with no gap and
    no overlap.  Unused slots hold FILLER."""
    words = [pack(*FILLER)] * (SHARDS * region_cap)
    used = [set() for _ in range(SHARDS)]
    for k, (mlen, tile, evs) in enumerate(chunks):
        shard, slot = deal(k, mlen, tile, len(evs))
        assert 0 <= shard < SHARDS and 0 <= slot and slot + len(evs) <= region_cap, (k, shard, slot, len(evs), region_cap)
        for j, e in enumerate(evs):
            assert slot + j not in used[shard], (k, shard, slot + j)
            used[shard].add(slot + j)
            words[shard * region_cap + slot + j] = pack(*e)
    counters = [len(u) for u in used]
    for shard, u in enumerate(used):
        assert u == set(range(len(u))), f"region {shard} has a gap"
    return np.array(words, dtype="<u8"), np.array(counters, dtype="<u4")


def layout(truth_runs, region_cap, deal):
    """the events of truth_runs, cut into (motif, tile) chunks and placed as `deal` names (see place)"""
    return place(chunks_of(events_of(truth_runs)), deal, region_cap)


def appended(chunks, shard_of, order=None):
    """a deal: the chunks are appended to their regions in `order` (a list of chunk numbers, default 0, 1, ...), chunk k to region
    shard_of[k]"""
    fill = [0] * SHARDS
    where = {}
    for k in (range(len(chunks)) if order is None else order):
        where[k] = (shard_of[k], fill[shard_of[k]])
        fill[shard_of[k]] += len(chunks[k][2])
    assert len(where) == len(chunks)
    return lambda k, mlen, tile, n: where[k]


# ------------------------------------------------------------------------------------------------------------------ the legacy pair
def dense_and_table(words, counters, region_cap, m_lo, nm, length):
    """What compact_events_kernel and chunk_table_kernel must leave: -> (dense, summary, overflow, table, status).  dense: the regions
    one after the other in region order, each cut at region_cap; summary its length; overflow 1 if any counter exceeds region_cap;
    table[motif - m_lo][tile] = [index of the chunk's first event in dense + 1, index past its last] (0, 0 without one), a chunk being a
    longest stretch of dense with one (motif, tile); status bit 0: an event whose motif or tile is outside the launch, bit 1: a
    (motif, tile) with more than one chunk (its table entry is then not defined)."""
    dense, overflow = [], 0
    for shard in range(SHARDS):
        kept = min(int(counters[shard]), region_cap)
        overflow |= int(counters[shard]) > region_cap
        dense.extend(int(w) for w in words[shard * region_cap:shard * region_cap + kept])
    ntile = ntile_of(length)
    table = np.zeros((nm, ntile, 2), "<u4")
    status, prev = 0, None
    for i, w in enumerate(dense):
        pos, mlen, _ = unpack(w)
        key = (mlen, pos // TILE)
        if not (m_lo <= mlen < m_lo + nm and key[1] < ntile):
            status |= 1
        else:
            entry = table[mlen - m_lo][key[1]]
            if key != prev:
                if entry[0]:
                    status |= 2
                entry[0] = i + 1
            entry[1] = i + 1
        prev = key
    return np.array(dense, dtype="<u8"), len(dense), overflow, table, status


def motif_streams(dense, table, m_lo, nm):
    """the events of each motif as the table lists them: chunk after chunk in tile order -> (pos, mlen, kind) list, motif-major"""
    out = []
    for mi in range(nm):
        for first1, end in table[mi]:
            if first1:
                out.extend(unpack(w) for w in dense[int(first1) - 1:int(end)])
    return out


def as_records(rows):
    return np.array([tuple(r) for r in rows], dtype=RUN_DT).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------------- cases
def case(name, m_lo, m_hi, length, words, counters, region_cap, stream, own=WHOLE, flags=0):
    """(the generators below build their cases once; the tests read them and leave them unchanged)
    stream: the events the kernels may read -- the first min(counter, region_cap) of every region -- in (motif, position) order (None
    for a malformed case); flags: the PAIR_* bits the pairing must report"""
    return {"name": name, "m_lo": m_lo, "m_hi": m_hi, "nm": m_hi - m_lo + 1, "length": length, "ntile": ntile_of(length), "events": words,
            "counters": counters, "region_cap": region_cap, "stream": stream, "own_lo": own[0], "own_hi": own[1], "pos_offset": own[2],
            "flags": flags}


def truth_case(name, m_lo, m_hi, length, truth, region_cap, shard_of, order=None, own=WHOLE):
    chunks = chunks_of(events_of(truth))
    words, counters = layout(truth, region_cap, appended(chunks, shard_of(chunks) if callable(shard_of) else shard_of, order))
    return case(name, m_lo, m_hi, length, words, counters, region_cap, events_of(truth), own)


def scrambled(n, seed, among=SHARDS):
    """n different regions, in an order fixed by the seed"""
    return random.Random(seed).sample(range(among), n)


SHARD_M = (2, 20)
SHARD_LENGTH = 5 * TILE


@functools.lru_cache(maxsize=None)
def shard_truth():
    """38 runs over motifs 2, 7, 13 and 20 of a record of 5 tiles (6 table columns): all three END kinds; runs inside a tile and across one
    and two tile edges; motif 13's run from 10000 is the last event of its chunk and ends as the first event of the chunk three tiles on;
    motif 13's last run is open to the end of the record"""
    rng = random.Random(20)
    runs = []
    for mlen, n in ((2, 12), (20, 11)):
        cuts = sorted(rng.sample(range(1, SHARD_LENGTH // 8), 2 * n))            # distinct multiples of 8, so that +-1 stays distinct
        runs += [(8 * cuts[2 * j], 8 * cuts[2 * j + 1], mlen, j % 2) for j in range(n)]
    runs += [(100, 200, 7, 1), (900, 901, 7, 0), (16000, 16500, 7, 0), (20000, 40000, 7, 1), (40008, 40016, 7, 0), (49000, 49152 + 30, 7, 0),
             (49152 + 40, 65536 - 1, 7, 1), (65536, 65540, 7, 0), (65600, 70000, 7, 1), (70100, 70200, 7, 0), (81000, 81900, 7, 1)]
    runs += [(200, 900, 13, 0), (10000, 3 * TILE + 50, 13, 1), (3 * TILE + 100, 3 * TILE + 300, 13, 0), (4 * TILE + 5, SHARD_LENGTH, 13, 2)]
    runs.sort(key=lambda r: (r[2], r[0]))
    chunks = chunks_of(events_of(runs))
    assert {r[3] for r in runs} == {0, 1, 2} and any(c[2][0][2] != S for c in chunks) and len(chunks) <= SHARDS
    return runs


@functools.lru_cache(maxsize=None)
def shard_cases():
    truth = shard_truth()
    chunks = chunks_of(events_of(truth))
    sizes = [len(c[2]) for c in chunks]
    n, total = len(chunks), sum(sizes)
    mk = lambda name, cap, shard_of, order=None: truth_case(name, *SHARD_M, SHARD_LENGTH, truth, cap, shard_of, order)
    out = [mk("own_shard_scrambled", max(sizes), scrambled(n, 1)),
           mk("all_in_shard_63", total, [63] * n, scrambled(n, 2, among=n))]
    # region 63 exactly full with the three largest chunks (one at slot 0, one ending at slot region_cap - 1: the last word of the buffer);
    # region 0 starts with a chunk at slot 0 as well; the rest wherever it fits next
    big = sorted(range(n), key=lambda k: -sizes[k])[:3]
    cap = sum(sizes[k] for k in big)
    shard_of, fill, nxt = [None] * n, [0] * SHARDS, 0
    for k in big:
        shard_of[k] = 63
    for k in range(n):
        if shard_of[k] is None:
            while fill[nxt] + sizes[k] > cap:
                nxt += 1
            shard_of[k] = nxt
            fill[nxt] += sizes[k]
    c = mk("full_region", cap, shard_of, big + [k for k in range(n) if k not in big])
    assert int(c["counters"][63]) == cap
    out.append(c)
    # motif 13: START 10000 is the last event of a chunk in region 5, its END opens a chunk in region 2, three tiles on
    a = next(k for k, ch in enumerate(chunks) if ch[0] == 13 and ch[1] == 0)
    b = next(k for k, ch in enumerate(chunks) if ch[0] == 13 and ch[1] == 3)
    assert chunks[a][2][-1] == (10000, 13, S) and chunks[b][2][0] == (3 * TILE + 50, 13, EN) and chunks[a + 1] is chunks[b]
    shard_of = [5 if k == a else 2 if k == b else 10 + k % 7 for k in range(n)]
    out.append(mk("start_in_shard_5_end_in_shard_2", total, shard_of, [k for k in range(n) if k != b] + [b]))
    for seed in range(8):
        rng = random.Random(100 + seed)
        order = list(range(n))
        rng.shuffle(order)
        out.append(mk(f"random_deal_{seed}", total, [rng.randrange(SHARDS) for _ in range(n)], order))
    return out


def single_event_case():
    """region_cap 1: 64 events, every one a chunk of its own, one per region"""
    truth = [(t * TILE + 50 + m, (t + 1) * TILE + 20 + m, m, (t // 2 + m) % 2) for m in range(2, 12) for t in (0, 2)]
    truth += [(4 * TILE + 50 + m, SHARD_LENGTH, m, 2) for m in range(2, 12)]              # (tile 5 holds the end of the record only)
    truth += [(2 * TILE + 7, 3 * TILE + 9, 19, 0), (77, SHARD_LENGTH, 20, 2)]
    truth.sort(key=lambda r: (r[2], r[0]))
    c = truth_case("region_cap_1", *SHARD_M, SHARD_LENGTH, truth, 1, scrambled(64, 3))
    assert list(c["counters"]) == [1] * 64
    return c


def clamp_case():
    """region 0 overflowed by 7: its region_cap slots hold a whole well-formed stream; region 1 (counter 0) holds events of motif 25,
    which the launch does not have -- the words a read past the cap would meet"""
    truth = [r for r in shard_truth() if r[2] in (2, 7)]
    chunks = chunks_of(events_of(truth))
    cap = sum(len(c[2]) for c in chunks)
    words, counters = layout(truth, cap, appended(chunks, [0] * len(chunks), scrambled(len(chunks), 4, among=len(chunks))))
    for j in range(cap):
        words[cap + j] = pack(100 + 10 * j, 25, j % 2)
    counters[0] = cap + 7
    return case("clamp", *SHARD_M, SHARD_LENGTH, words, counters, cap, events_of(truth))


@functools.lru_cache(maxsize=None)
def seam_cases():
    """positions 16383 / 16384 / 16385 as START and as END; runs across 0, 1, 2 and ntile - 2 empty tiles; chunks that are one START or one
    END; a chunk that opens with an END and goes on with 300 runs; the end of the record on a tile edge and one base behind it"""
    out = []
    for name, length in (("seams_length_on_tile_edge", 8 * TILE), ("seams_length_one_past_tile_edge", 8 * TILE + 1)):
        T = TILE
        truth = [(T - 1, T, 2, 0), (T, T + 1, 3, 1), (16000, T - 1, 4, 0), (T + 1, T + 16, 4, 1), (100, T, 5, 0), (100, T + 1, 6, 1),
                 (T - 10, T + 10, 7, 0), (T - 10, 2 * T + 10, 8, 1), (10, 3 * T + 5, 9, 0), (T - 1, length, 10, 2),
                 (T - 5, T + 3, 11, 0)] + [(T + 10 + 40 * k, T + 30 + 40 * k, 11, k % 2) for k in range(300)]
        truth.sort(key=lambda r: (r[2], r[0]))
        chunks = chunks_of(events_of(truth))
        assert max(len(c[2]) for c in chunks) == 601 and ntile_of(length) == 9
        out.append(truth_case(name, *SHARD_M, length, truth, 601, scrambled(len(chunks), 5)))
    return out


def _entry_runs(entries, nm, ntile, m_lo):
    """1 + k % 3 short runs in every table entry k of `entries` (entry = (motif - m_lo) * ntile + tile)"""
    truth = []
    for k in sorted(set(entries)):
        mi, tile = divmod(k, ntile)
        assert mi < nm
        truth += [(tile * TILE + 100 + 200 * j, tile * TILE + 150 + 200 * j, m_lo + mi, (k + j) % 2) for j in range(1 + k % 3)]
    return truth


@functools.lru_cache(maxsize=None)
def prefix_cases():
    """tables of 1023, 1024, 1025, 2049 and 4 * 1024 + 3 entries (the three-pass prefix sum works in blocks of 1024, four entries per thread,
    64 threads per wave): runs in the first and last entry of every block, in entries 3, 4, 255, 256, 257 of every block, and in the last"""
    out = []
    for m_lo, nm, ntile in ((2, 11, 93), (2, 16, 64), (2, 25, 41), (2, 3, 683), (5, 1, 4099)):
        entries = nm * ntile
        want = [b + j for b in range(0, entries, 1024) for j in (0, 3, 4, 255, 256, 257, 1023)] + [entries - 1]
        truth = _entry_runs([k for k in want if k < entries], nm, ntile, m_lo)
        chunks = chunks_of(events_of(truth))
        out.append(truth_case(f"prefix_{entries}", m_lo, m_lo + nm - 1, (ntile - 1) * TILE + 1000, truth, 64,
                              [k % SHARDS for k in range(len(chunks))], scrambled(len(chunks), entries, among=len(chunks))))
    return out


@functools.lru_cache(maxsize=None)
def carry_cases():
    """989 motifs: tables of 255, 256, 257 and 513 blocks of 1024 (pair_scan_partials_kernel takes 256 block sums at a time), a dozen runs:
    in the first block, the 256th, the 257th (where the table has them) and the last entry"""
    out = []
    m_lo, nm = 2, 989
    for ntile in (264, 265, 266, 531):
        entries = nm * ntile
        want = [0, 5, 1023, 255 * 1024, 255 * 1024 + 1023, 256 * 1024, 256 * 1024 + 1, entries - 1024, entries - 1]
        truth = _entry_runs([k for k in want if k < entries], nm, ntile, m_lo)
        chunks = chunks_of(events_of(truth))
        out.append(truth_case(f"carry_{(entries + 1023) // 1024}_blocks", m_lo, m_lo + nm - 1, (ntile - 1) * TILE + 1000, truth, 8,
                              scrambled(len(chunks), ntile)))
    return out


@functools.lru_cache(maxsize=None)
def grid_stride_cases():
    """one region with 16384, 16385 and 40001 events of one motif (the kernels that walk a region give it at most 64 blocks of 256 threads):
    short runs over many tiles.  A well-formed stream has an even number of events, so at the odd sizes the END of the last run, a chunk
    of its own, lies in region 0; every other region is empty."""
    out = []
    for n in (16384, 16385, 40001):
        runs = (n + 1) // 2
        truth = [(100 * k + 3, 100 * k + 60, 2, k % 2) for k in range(runs - 1)]
        last_tile = (100 * runs) // TILE + 1
        truth.append((last_tile * TILE - 9, last_tile * TILE + 4, 2, 0))
        chunks = chunks_of(events_of(truth))
        assert chunks[-1][2] == [(last_tile * TILE + 4, 2, E0)]
        shard_of = [37] * len(chunks)
        if n % 2:
            shard_of[-1] = 0
        c = truth_case(f"grid_stride_{n}", 2, 2, (last_tile + 1) * TILE, truth, n, shard_of, scrambled(len(chunks), n, among=len(chunks)))
        assert int(c["counters"][37]) == n and int(c["counters"].sum()) == n + n % 2
        out.append(c)
    return out


def own_cuts(truth, length):
    """every run's START, START +- 1, END, END +- 1, inside 0 .. length + 1, ascending"""
    return sorted({p + d for r in truth for p in r[:2] for d in (-1, 0, 1) if 0 <= p + d <= length + 1})


def own_ranges(truth, length):
    """(own_lo, own_hi) with both ends on own_cuts: from the start of the record to every cut, from every cut to its end, and from
    every cut to the cut seven further on; then the empty ranges and the whole record"""
    cuts = own_cuts(truth, length)
    out = [(0, c) for c in cuts] + [(c, length + 1) for c in cuts] + [(c, cuts[i + 7]) for i, c in enumerate(cuts[:-7])]
    return out + [(0, 0), (cuts[len(cuts) // 2],) * 2, (0, length + 1)]


def halves_cap_case():
    """every one of the 19 motifs has a run cut by own_lo and a run cut by own_hi: 38 halves, all the halves buffer holds; motif 9 has a
    whole run in between as well"""
    truth = [(100 + m, 1000 + m, m, m % 2) for m in range(2, 21)] + [(2000 + m, 3000 + m, m, (m + 1) % 2) for m in range(2, 21)]
    truth.append((1200, 1300, 9, 0))
    truth.sort(key=lambda r: (r[2], r[0]))
    chunks = chunks_of(events_of(truth))
    return truth_case("two_halves_per_motif", *SHARD_M, SHARD_LENGTH, truth, 8, scrambled(len(chunks), 6), own=(500, 2500, 0))


def covered_range_case():
    """motif 7's run 20000 .. 40000 covers the whole own range: a place holder and no half"""
    c = shard_cases()[0]
    return dict(c, name="run_covers_own_range", own_lo=25000, own_hi=30000)


@functools.lru_cache(maxsize=None)
def malformed_cases():
    """streams no scan may produce, over more than one region; `flags`: what the pairing must report (DUP_CHUNK: at least that)"""
    m_lo, m_hi, length = *SHARD_M, SHARD_LENGTH
    last = 5 * TILE
    specs = [
        # (another motif's chunk in a region between the two: side by side in the dense stream they would read as one chunk)
        ("dup_chunk_in_two_shards", DUP_CHUNK, [(3, 0, [(10, 3, S), (60, 3, E0)], 4), (5, 0, [(100, 5, S), (160, 5, E0)], 6),
                                                (3, 0, [(300, 3, S), (360, 3, E0)], 9)]),
        ("open_run_then_start_in_other_shard", NOT_ALTERNATING, [(3, 0, [(10, 3, S)], 1), (3, 1, [(20000, 3, S), (20100, 3, E0)], 0)]),
        ("start_in_last_tile_nothing_after", UNTERMINATED, [(3, 0, [(10, 3, S), (60, 3, E0)], 8), (3, 5, [(last, 3, S)], 3)]),
        # (an END in a later chunk is always above its START: chunks are cut by position; the rule can only be broken inside a chunk)
        ("end_not_above_its_start", NOT_ALTERNATING, [(5, 0, [(10, 5, S), (60, 5, E0)], 2), (3, 2, [(2 * TILE + 500, 3, S), (2 * TILE + 400, 3, E0)], 7)]),
        ("motif_outside_the_launch_in_shard_1", BAD_EVENT, [(3, 0, [(10, 3, S), (60, 3, E0)], 0), (25, 0, [(10, 25, S), (60, 25, E0)], 1)]),
    ]
    out = []
    for name, flags, placed in specs:
        chunks = [(m, t, evs) for m, t, evs, _ in placed]
        words, counters = place(chunks, appended(chunks, [p[3] for p in placed]), 2)
        out.append(case(name, m_lo, m_hi, length, words, counters, 2, None, flags=flags))
    return out


@functools.lru_cache(maxsize=None)
def well_formed_cases():
    """every well-formed case with a whole-record own range"""
    return shard_cases() + [single_event_case(), clamp_case()] + seam_cases() + prefix_cases() + carry_cases() + grid_stride_cases()


@functools.lru_cache(maxsize=None)
def cases_by_name():
    """every case, built once; the tests read them and leave them unchanged"""
    cases = well_formed_cases() + [halves_cap_case(), covered_range_case()] + malformed_cases()
    for c in cases:
        c["events"].setflags(write=False)
        c["counters"].setflags(write=False)
    by_name = {c["name"]: c for c in cases}
    assert len(by_name) == len(cases)
    return by_name
