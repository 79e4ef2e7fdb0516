"""The chunk contract stated with numpy (tests/test_sharded.py, tests/test_sharded_gpu.py, tests/test_sharded_cuts_gpu.py):
what one chunk of a record must return, cut out of the oracle's call lists and perfect runs of the whole record."""
import numpy as np

import pyevents
import ribbit_amd
from ribbit_amd import CALL_DT

SUBST_SPAN = lambda m: m // 3 if m > 30 else 10                                       # parse_substitute_shiftxor.cpp:423
ANCHORED_SPAN = lambda m: int(0.9 * m) if m >= 10 else (m if m > 6 else 10)           # parse_anchored_shiftxor.cpp:572-573


def spans(mlen, span):
    """span(m) of every entry of mlen (evaluated once per motif length)"""
    u, inv = np.unique(np.asarray(mlen, dtype=np.int64), return_inverse=True)
    return np.array([span(int(m)) for m in u], dtype=np.int64)[inv].reshape(-1)


def _chunk_calls(calls, length, own_lo, own_hi, last, span):
    """what ribbit_hip_stage_calls_chunk keeps of a stage's full call list for the chunk owning scan positions
    [own_lo, own_hi): the calls that pass the length filter, each with the largest end of the chunk's earlier calls;
    the largest end of any of its calls; the end-of-sequence calls (pos == length) if it is the last chunk"""
    loop = calls[(calls["pos"] < length) & (calls["pos"] >= own_lo) & (calls["pos"] < own_hi)]
    ends = loop["end"].astype(np.int64)
    seen = np.concatenate(([-1], np.maximum.accumulate(ends)[:-1])) if len(loop) else np.zeros(0, np.int64)
    keep = (loop["end"] - loop["start"]) >= spans(loop["mlen"], span)
    flush = calls[calls["pos"] >= length] if last else np.zeros(0, CALL_DT)
    return loop[keep].copy(), seen[keep].astype("<i4"), int(ends.max()) if len(loop) else -1, flush.copy()


def _chunk_runs(runs, own_lo, own_hi):
    """ribbit_hip_scan_perfect_chunk's records for the chunk: complete runs it owns, halves of the runs its edges cut"""
    s, e = runs["start"], runs["end"]
    s_own, e_own = (s >= own_lo) & (s < own_hi), (e >= own_lo) & (e < own_hi)
    whole = runs[s_own & (e < own_hi)].copy()
    hs = runs[s_own & (e >= own_hi)].copy(); hs["end"] = -1; hs["term"] = ribbit_amd.RUN_HALF_START
    he = runs[e_own & (s < own_lo)].copy(); he["start"] = -1; he["term"] = ribbit_amd.RUN_HALF_END + he["term"]
    return whole, np.concatenate((hs, he))


def oracle_runs(o, m_lo, m_hi):
    """the record's perfect runs, ordered by (mlen, start), from the events of an Oracle that has not run its perfect stage"""
    ev, cnt = pyevents.perfect_events(o, m_lo, m_hi)
    return ribbit_amd.host_perfect_runs_from_events(m_lo, m_hi, [ev], [cnt])
