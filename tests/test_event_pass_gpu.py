"""What the host side of every scan does around its kernel -- size the sharded event regions, launch, pair the START / END
events on the device, read the published counters, grow the regions and run again on overflow, check the pairing flags -- seen
from outside: the overflow retry on the paths test_perfect_gpu.py and test_scan_split_gpu.py do not reach, the event counts, which
timers are valid after which call, and the pairing hook.  One repeat-dense record of three tiles (a tile is 16,384 bases), motifs
2..20; every case takes a second or two.

Overflow is forced with a first capacity of 64 regions x 64 events.  A scan that leaves more than 4096 events must have overflowed
some region whichever way the kernels spread them over the 64 regions, so that is what is checked: on the CPU beforehand (pyevents:
the perfect scan's and the substitution stage's events exactly; of the anchored stage's the pass-streaks that are by themselves as
long as its group filter asks a group to be, which the filter cannot drop), and on the GPU afterwards (last_event_count / streaks)."""
import functools
import math

import numpy as np
import pytest

import pyevents
import ribbit_amd
from chunk_contract import ANCHORED_SPAN
from oracle_lib import Oracle
from ribbit_amd import STAGE_ANCHORED, STAGE_SUBST
from ribbit_amd.simulate import simulate_sequence

pytestmark = pytest.mark.gpu
M_LO, M_HI = 2, 20
BASES = 40_000
SMALL_CAP = 64 * 64
S, E0 = 0, 1


@functools.lru_cache(maxsize=None)
def _record():
    """the loci of a long simulated sequence (purity 90 to 97 %) back to back, each with 8 bases of its flanks: the plain
    sequence has a locus every two thousand bases and leaves a few hundred perfect events in 40,000 bases, not the 4096 an
    overflow needs"""
    seq, truth = simulate_sequence(16 * BASES, 11, M_LO, M_HI, 0.90, 0.97)
    parts, n = [], 0
    for s, e, _, _ in truth:
        parts.append(seq[max(0, s - 8):e + 8])
        n += len(parts[-1])
        if n >= BASES:
            break
    rec = b"".join(parts)[:BASES]
    assert len(rec) == BASES
    return rec


def _reach(m_hi):
    """(smallest left halo, smallest right halo) ribbit_hip_stage_calls_chunk accepts, as tests/test_sharded_cuts_gpu.py"""
    s = m_hi + 2
    return 2 * s + 56, 4 * s + 16


@functools.lru_cache(maxsize=None)
def _plans():
    """two chunks of the record, cut in the middle, each loaded with the tightest halos: (own_lo, own_hi, load_lo, load_hi)"""
    L, c = BASES, BASES // 2 + 5
    left, right = _reach(M_HI)
    return [(lo, hi, max(0, lo - left), min(L, hi + right)) for lo, hi in ((0, c), (c, L + 1))]


@functools.lru_cache(maxsize=None)
def _cpu_events(lo, hi):
    """(perfect events, substitution-stage window events) of record[lo:hi], counted on the CPU"""
    with Oracle(_record()[lo:hi], M_LO, M_HI) as o:
        return int(pyevents.perfect_events(o, M_LO, M_HI)[1].sum()), int(pyevents.window_events(o, M_LO, M_HI, 1)[1].sum())


@functools.lru_cache(maxsize=None)
def _cpu_anchored_events(lo, hi):
    """a lower bound of the anchored stage's filtered window events of record[lo:hi]: the filter drops a group of pass-streaks
    only if it spans fewer than min(span(m), 16 + 7) - 7 positions (kernels.h, GROUP_FILTER_MAX), so a streak that long stays"""
    with Oracle(_record()[lo:hi], M_LO, M_HI) as o:
        o.run_perfect(); o.run_subst(); o.run_anchor_planes()
        ev, cnt = pyevents.window_events(o, M_LO, M_HI, 2)
    n, off = 0, 0
    for m, c in zip(range(M_LO, M_HI + 1), cnt):
        pos = (ev[off:off + int(c)] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        off += int(c)
        n += 2 * int(((pos[1::2] - pos[0::2]) >= min(ANCHORED_SPAN(m), 16 + 7) - 7).sum())
    return n


@pytest.fixture(scope="module")
def pair():
    """(scanner with the default capacity, scanner whose first capacity is 64 x 64 events)"""
    with ribbit_amd.Scanner(M_LO, M_HI) as ref, ribbit_amd.Scanner(M_LO, M_HI) as sc:
        sc.debug_set_event_capacity(SMALL_CAP)
        yield ref, sc


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- overflow retry ---------------------------------------------------------------------------------------------------

def test_host_paired_partial_runs_survive_an_overflow(pair):
    ref, sc = pair
    seq = _record()
    assert _cpu_events(0, BASES)[0] > SMALL_CAP
    a, b = BASES // 3 + 1, 2 * BASES // 3 + 2
    out = []
    for s in (ref, sc):
        s.load_record(seq)
        out.append(s.perfect_runs_partial(a, b, 7))
        assert s.last_event_count() == _cpu_events(0, BASES)[0] > SMALL_CAP
    assert len(out[0][0]) > 0
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])


def test_perfect_chunk_with_a_cut_run_survives_an_overflow(pair):
    ref, sc = pair
    seq = _record()
    assert _cpu_events(0, BASES)[0] > SMALL_CAP
    ref.load_record(seq)
    runs = ref.scan_perfect_runs()
    # the own range starts inside the longest run and ends inside the longest of the runs that lie beyond it
    first = runs[np.argmax(runs["end"] - runs["start"])]
    beyond = runs[runs["start"] > first["end"]]
    if len(beyond) == 0:
        beyond = runs[runs["end"] < first["start"]]
    second = beyond[np.argmax(beyond["end"] - beyond["start"])]
    a, b = sorted(int(r["start"] + r["end"]) // 2 for r in (first, second))
    assert a < b
    out = []
    for s in (ref, sc):
        s.load_record(seq)
        rec, halves = s.scan_perfect_chunk(a, b, 3)
        out.append((np.array(rec), halves))
        assert s.last_event_count() > SMALL_CAP
    assert len(out[0][1]) >= 2, "both ends of the own range cut a run"
    assert _same(out[0][0], out[1][0]) and _same(out[0][1], out[1][1])


@pytest.mark.parametrize("stage", [STAGE_SUBST, STAGE_ANCHORED], ids=["subst", "anchored"])
def test_window_stage_of_two_chunks_survives_an_overflow(pair, stage):
    ref, sc = pair
    seq = _record()
    for own_lo, own_hi, load_lo, load_hi in _plans():
        assert (_cpu_events(load_lo, load_hi)[1] if stage == STAGE_SUBST else _cpu_anchored_events(load_lo, load_hi)) > SMALL_CAP
        out = []
        for s in (ref, sc):
            s.load_record(seq[load_lo:load_hi])
            out.append(s.stage_calls_chunk(stage, own_lo - load_lo, own_hi - load_lo, load_lo, BASES))
            assert s.last_event_count() == 2 * out[-1]["streaks"] > SMALL_CAP
        want, got = out
        assert len(want["calls"]) > 0
        for k in ("calls", "flush"):
            assert _same(want[k], got[k]), k
        assert (want["pend"] is None) == (got["pend"] is None) and (want["pend"] is None or _same(want["pend"], got["pend"]))
        assert (want["tail_pend"], want["inexact"], want["streaks"]) == (got["tail_pend"], got["inexact"], got["streaks"])


# ---- event counts -----------------------------------------------------------------------------------------------------

def test_event_counts_after_every_kind_of_scan(pair):
    ref, _ = pair
    ref.load_record(_record())
    runs = ref.scan_perfect_runs()
    assert len(runs) > 0 and ref.last_event_count() == 2 * len(runs)
    ref.load_record(_record())
    ref.scan_perfect_begin()
    runs2, _ = ref.scan_perfect_end()
    assert ref.last_event_count() == 2 * len(runs2) == 2 * len(runs)
    assert len(ref.subst_calls()) > 0
    n = ref.last_event_count()
    assert n > 0 and n % 2 == 0
    assert len(ref.anchored_calls()) > 0
    n = ref.last_event_count()
    assert n > 0 and n % 2 == 0


# ---- timer state ------------------------------------------------------------------------------------------------------

def _works(sc, what):
    ms = sc.timing_ms(what)
    assert math.isfinite(ms) and ms >= 0, (what, ms)


def _raises(sc, what, match=None):
    with pytest.raises(ribbit_amd.RibbitHipError, match=match):
        sc.timing_ms(what)


def test_timers_of_the_pack_and_the_perfect_scan():
    seq = _record()
    with ribbit_amd.Scanner(M_LO, M_HI) as sc:
        sc.load_record(seq)
        _works(sc, 0); _raises(sc, 1); _raises(sc, 2)
        sc.scan_perfect_begin()
        sc.scan_perfect_end_device()
        _works(sc, 1); _raises(sc, 2)
        sc.scan_perfect_begin()
        sc.scan_perfect_end()
        _works(sc, 1); _works(sc, 2)
        _raises(sc, 10, match="what must be 0..9")
        sc.set_timing(False)
        sc.scan_perfect_runs()
        for what in (0, 1, 2):
            _raises(sc, what)


def test_timers_of_the_window_stages():
    seq = _record()
    with ribbit_amd.Scanner(M_LO, M_HI) as sc:
        sc.load_record(seq)
        _raises(sc, 6)
        sc.processShiftXORswithSubstitutions()
        _works(sc, 6)
        sc.load_record(seq)
        sc.processShiftXORsAnchored()
        for what in (6, 7, 8, 9):
            _works(sc, what)


def test_timers_of_the_anchored_kernels_after_an_overflow(pair):
    _, sc = pair
    assert _cpu_anchored_events(0, BASES) > SMALL_CAP
    sc.load_record(_record())
    sc.processShiftXORsAnchored()
    assert sc.last_event_count() > SMALL_CAP          # the anchored stage's window scan ran twice, its planes kernel once
    _works(sc, 7); _raises(sc, 8); _raises(sc, 9)


# ---- the pairing hook -------------------------------------------------------------------------------------------------

def _ev(pos, m, kind):
    return np.uint64(pos) | (np.uint64(m) << np.uint64(32)) | (np.uint64(kind) << np.uint64(48))


def test_pairing_hook_on_a_hand_made_stream(pair):
    ref, _ = pair
    runs, flags = ref.debug_pair_events(np.array([_ev(10, 3, S), _ev(60, 3, E0), _ev(200, 3, S), _ev(900, 3, E0), _ev(100, 7, S), _ev(150, 7, E0)],
                                                 dtype="<u8"), 3 * 16384)
    assert flags == 0
    assert [tuple(int(x) for x in r) for r in runs] == [(10, 60, 3, 0), (200, 900, 3, 0), (100, 150, 7, 0)]
    runs, flags = ref.debug_pair_events(np.array([_ev(10, 3, S), _ev(40, 3, S), _ev(60, 3, E0)], dtype="<u8"), 3 * 16384)
    assert flags & 4, flags
