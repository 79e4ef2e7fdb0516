"""GPU tests of the scan kernels' motif split (run with -m gpu on an MI355X).

Each scan kernel splits the motif range over gridDim.y blocks, and each block deals its motifs to 4 waves: round-robin in the
perfect, substitution-window and composed-plane window kernels, in contiguous groups in the anchored planes kernel.  The
automatic split is chosen from the record length, so short test records and chromosomes run different decompositions (candidate
queue flushes across motifs, the cached shifted words at multiples of 32, the anchored kernel's five-shift ring and its warm-up
shifts).  Here the split is forced through ribbit_hip_debug_set_scan_split and every stage's output must equal the CPU oracle's
under every split, bit for bit: perfect / substitution / anchored calls, every composed plane, the three seed lists, the dispatch
order and the guard hits.  The oracle runs once per record.  The second half walks the anchored kernel's tile edges at every
halo-lane count (device_planes.h: anchored_halo_lanes).
"""
import functools

import numpy as np
import pytest

import ribbit_amd
from ribbit_amd import SCAN_ALL, SCAN_ANCHORED, SCAN_PERFECT, SCAN_SUBST, SCAN_XA_WINDOW
from cases import HALO_STEP_M_HI, SPLIT_RANGES, anchored_tile_bases, halo_step_record, scan_split_record
from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle

pytestmark = pytest.mark.gpu

KERNELS = (SCAN_PERFECT, SCAN_SUBST, SCAN_ANCHORED, SCAN_XA_WINDOW)
SPLIT_LENGTHS = {(2, 100): 120_000, (2, 14): 60_000, (30, 200): 100_000, (100, 500): 60_000, (500, 990): 100_000}
TILE_BASES = 16384


def _splits(nm):
    return sorted({min(v, nm) for v in (1, 2, 3, 4, 5, 6, 7, 8, 9, 20, 21, 31, 32, 33)} | {max(nm - 1, 1), nm})


def _auto_split(kernel, length, m_lo, m_hi):
    """the launchers' automatic choice (kernels.hip: scan_split) -> (gridDim.y, motifs per block)"""
    nm = m_hi - m_lo + 1
    nwords = length // 32 + 1
    if kernel == SCAN_ANCHORED:
        tw = anchored_tile_bases(m_hi) // 32
        ntiles = (nwords + tw - 1) // tw
        want, max_y = (1024 + ntiles - 1) // ntiles, (nm + 31) // 32
    else:
        ntiles = (nwords + TILE_BASES // 32 - 1) // (TILE_BASES // 32)
        want, max_y = (2048 + ntiles - 1) // ntiles, (nm + 3) // 4
    gy = max(1, min(want, max_y))
    mpb = (nm + gy - 1) // gy
    return (nm + mpb - 1) // mpb, mpb


def _expected_split(kernel, forced, length, m_lo, m_hi):
    nm = m_hi - m_lo + 1
    if forced == 0:
        return _auto_split(kernel, length, m_lo, m_hi)
    mpb = min(forced, nm)
    return (nm + mpb - 1) // mpb, mpb


def _packed_words(bits, nwords):
    """0/1 bytes of a plane -> little-endian uint32 words, zero beyond the record"""
    out = np.zeros(nwords * 4, np.uint8)
    packed = np.packbits(bits, bitorder="little")
    out[: len(packed)] = packed
    return out.view("<u4")


class Want:
    """everything the oracle says about one record, computed once"""

    def __init__(self, seq, m_lo, m_hi):
        self.seq, self.m_lo, self.m_hi = seq, m_lo, m_hi
        self.nwords = len(seq) // 32 + 1
        with Oracle(seq, m_lo, m_hi) as o:
            o.run_all()
            self.calls = [o.calls(w).view("<i4").copy() for w in (LIST_PERFECT, LIST_SUBST, LIST_ANCHORED)]
            self.seeds = [o.seeds(w).view("<i4").copy() for w in (LIST_PERFECT, LIST_SUBST, LIST_ANCHORED)]
            self.dispatch = o.dispatch().view("<i4").copy()
            self.guard_hits = o.guard_hits()
            self.planes = np.stack([_packed_words(o.plane(m), self.nwords) for m in range(m_lo, m_hi + 1)])
        # the bits of the last word beyond the record are not part of any plane
        self.mask = _packed_words(np.ones(len(seq), np.uint8), self.nwords)


@functools.lru_cache(maxsize=None)
def _want_split_record(m_lo, m_hi):
    return Want(scan_split_record(m_lo, m_hi, SPLIT_LENGTHS[(m_lo, m_hi)], m_lo + m_hi), m_lo, m_hi)


def _check_all(sc, want, splits, what):
    """load the record, run every stage, compare everything with the oracle; `splits`: per kernel, the forced
    motifs per block (0 = automatic) the launches must report"""
    L, m_lo, m_hi = len(want.seq), want.m_lo, want.m_hi
    # The composed planes stay in the handle's buffer from one load to the next: fill it with those of an all-A record of the
    # same length (all ones) first, so that a plane this load's kernel fails to write cannot pass as the previous split's.
    # The fill runs at one motif per block, not under the split being tested (which would skip the same planes), and is checked.
    sc.debug_set_scan_split(SCAN_ANCHORED, 1)
    sc.load_record(b"A" * L)
    sc.adopt_dispatch(np.zeros(0, ribbit_amd.SEED_DT))         # the planes kernel alone
    assert ((sc.xa_words(0, want.nwords) & want.mask) == want.mask).all(), f"{what}: the all-A record's planes are not all ones"
    sc.debug_set_scan_split(SCAN_ANCHORED, splits[SCAN_ANCHORED])
    sc.load_record(want.seq)
    # seed lists first: the anchored window scan then runs with its group filter (the compact form the merges use)
    perfect, subst, anchored = sc.processShiftXORsAnchored()
    for k in KERNELS:
        assert sc.debug_last_scan_split(k) == _expected_split(k, splits[k], L, m_lo, m_hi), f"{what}: kernel {k} launched another split"
    assert np.array_equal(perfect.view("<i4"), want.seeds[0]), f"{what}: perfect seeds"
    assert np.array_equal(subst.view("<i4"), want.seeds[1]), f"{what}: substitution seeds"
    assert np.array_equal(anchored.view("<i4"), want.seeds[2]), f"{what}: anchored seeds"
    assert np.array_equal(sc.dispatch_seeds().view("<i4"), want.dispatch), f"{what}: dispatch order"
    assert sc.guard_hits() == want.guard_hits, f"{what}: guard hits"
    # the full call lists (the anchored window scan again, without the filter)
    assert np.array_equal(sc.perfect_calls().view("<i4"), want.calls[0]), f"{what}: perfect calls"
    assert np.array_equal(sc.subst_calls().view("<i4"), want.calls[1]), f"{what}: substitution calls"
    assert np.array_equal(sc.anchored_calls().view("<i4"), want.calls[2]), f"{what}: anchored calls"
    for k in KERNELS:
        assert sc.debug_last_scan_split(k) == _expected_split(k, splits[k], L, m_lo, m_hi), f"{what}: kernel {k} launched another split"
    # every composed plane XA_m, m_lo..m_hi, as the planes kernel of this load wrote it (the same words plane_bits reads)
    got = sc.xa_words(0, want.nwords) & want.mask
    bad = np.nonzero((got != want.planes).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: composed planes differ at motifs {(bad + m_lo)[:10].tolist()}"


def _set_all(sc, v):
    sc.debug_set_scan_split(SCAN_ALL, v)
    return {k: v for k in KERNELS}


@pytest.mark.parametrize("m_lo,m_hi", SPLIT_RANGES, ids=[f"m{a}_M{b}" for a, b in SPLIT_RANGES])
def test_every_motif_split_matches_the_oracle(m_lo, m_hi):
    want = _want_split_record(m_lo, m_hi)
    nm = m_hi - m_lo + 1
    with ribbit_amd.Scanner(m_lo, m_hi) as sc:
        _check_all(sc, want, _set_all(sc, 0), "automatic split")
        for v in _splits(nm):
            _check_all(sc, want, _set_all(sc, v), f"{v} motifs per block")
        # one kernel with the whole range in one block (the anchored kernel: 1/4 of it per wave), the others automatic
        for k in KERNELS:
            splits = _set_all(sc, 0)
            sc.debug_set_scan_split(k, nm)
            splits[k] = nm
            _check_all(sc, want, splits, f"kernel {k} at {nm} motifs per block")


def test_event_overflow_retry_under_forced_splits():
    """The split decides which event shard each wave writes to: a first event capacity far too small must still give the
    same lists after the overflow retry, under every split."""
    want = _want_split_record(2, 100)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.debug_set_event_capacity(64 * 64)
        for v in (1, 5, 33, 99):
            _check_all(sc, want, _set_all(sc, v), f"capacity 4096, {v} motifs per block")


def test_split_override_arguments():
    with ribbit_amd.Scanner(2, 14) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError):
            sc.debug_set_scan_split(SCAN_ALL, -1)
        with pytest.raises(ribbit_amd.RibbitHipError):
            sc.debug_set_scan_split(SCAN_ALL + 1, 3)
        with pytest.raises(ribbit_amd.RibbitHipError):
            sc.debug_last_scan_split(SCAN_ALL)
        sc.load_record(b"ACGT" * 300)
        assert all(sc.debug_last_scan_split(k) == (0, 0) for k in KERNELS)      # nothing has run on this record yet
        sc.debug_set_scan_split(SCAN_SUBST, 1000)                                 # clamped to the 13 motifs
        sc.subst_calls()
        assert sc.debug_last_scan_split(SCAN_SUBST) == (1, 13)


HALO_CASES = [(m_hi, k * anchored_tile_bases(m_hi) + d) for m_hi in HALO_STEP_M_HI for k in (1, 2) for d in (-1, 0, 1)]


@pytest.mark.parametrize("m_hi,length", HALO_CASES, ids=[f"M{m}_L{n}" for m, n in HALO_CASES])
def test_anchored_tile_edges_at_every_halo_lane_count(m_hi, length):
    """Records of k*T - 1, k*T, k*T + 1 bases (T: the anchored tile at this max_motif, k = 1, 2) on both sides of every step
    of the halo-lane count, with a degenerate repeat of period near m_hi across each tile edge and a run open at the end."""
    m_lo = m_hi - 40
    want = Want(halo_step_record(m_hi, length), m_lo, m_hi)
    with ribbit_amd.Scanner(m_lo, m_hi) as sc:
        _check_all(sc, want, _set_all(sc, 0), "automatic split")
        _check_all(sc, want, _set_all(sc, 7), "7 motifs per block")
