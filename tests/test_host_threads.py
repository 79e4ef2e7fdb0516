"""Every team of host threads goes through one helper (ribbit_amd/csrc/host_threads.h): a thread that cannot start leaves its
part to the calling thread and the result is the same; a part that throws ends the entry point with RIBBIT_E_NOMEM and a
message -- not the calling process -- with every thread joined, so that the next call is right again.

ribbit_host_debug_thread_faults injects both faults into every team of two parts or more and counts them.  Each case is a
host-only entry point (no GPU) in a child interpreter with RIBBIT_THREADS=4, so that a regression shows as the child's exit
status (134: terminate called ...) and not as the death of pytest.  The inputs are sized so that a team of three or more
forms (the second thread start, and part 1, exist); every step asserts that the hook fired, so a case whose team did not form
fails instead of passing untested.  What a call must return is the oracle's answer or the numpy statement of the contract,
never another run of the library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROLOGUE = r"""
import ctypes as C, sys
sys.path[:0] = [%(root)r, %(root)r + "/tests"]
import numpy as np
import ribbit_amd
L = ribbit_amd.load_library()
faults = L.ribbit_host_debug_thread_faults

def exercise(call, check):
    # call() -> the entry point's result (RibbitHipError on a status); check(result) compares it with what it must be
    for start in (0, 1):
        faults(start, -1)
        got = call()
        fired = faults(-1, -1)
        assert fired > 0, "thread start %%d was never reached: no team large enough formed" %% start
        check(got)
        print("refused-start-%%d-same-result" %% start)
    for part in (0, 1):
        faults(-1, part)
        try:
            call()
        except ribbit_amd.RibbitHipError as e:
            msg = str(e)
        else:
            raise AssertionError("part %%d threw and the call returned a result" %% part)
        fired = faults(-1, -1)
        assert fired > 0, "part %%d never ran in a team of two or more" %% part
        assert " error -4: " in msg and "out of host memory" in msg, msg          # RIBBIT_E_NOMEM and its message
        assert "out of host memory" in L.ribbit_hip_last_error().decode()
        check(call())                                                              # the hook off: nothing left joinable or locked
        assert faults(-1, -1) == 0
        print("thrown-in-part-%%d-nomem-then-right" %% part)
"""

ORACLE_CASE = r"""
from cases import simulated_cases
from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle
name, seq, m_lo, m_hi = [c for c in simulated_cases() if c[0] == "sim_cfg2_120k"][0]
"""

CASES = {
    # refine_to_bed's chunks of seeds on the threads (refine.cpp); 8,701 dispatched seeds
    "refine_bed": ORACLE_CASE + r"""
with Oracle(seq, m_lo, m_hi) as o:
    o.run_all()
    d = o.dispatch()
    xa, stride = ribbit_amd.pack_bit_planes([o.plane(m) for m in range(m_lo, m_hi + 1)], len(seq))
    want = o.refine_bed("x")
assert len(d) >= 2048 and want.count("\n") > 500
def check(got):
    assert got == want
exercise(lambda: ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, d, "x"), check)
""",
    # the range-parallel merges and the scans that prepare them (parallel_merge.cpp), cut wherever a cut is valid
    "replay_calls": ORACLE_CASE + r"""
with Oracle(seq, m_lo, m_hi) as o:
    o.run_all()
    calls = [o.calls(k).copy() for k in (LIST_PERFECT, LIST_SUBST, LIST_ANCHORED)]
    want = {"perfect": o.seeds(LIST_PERFECT).copy(), "subst": o.seeds(LIST_SUBST).copy(), "anchored": o.seeds(LIST_ANCHORED).copy(),
            "dispatch": o.dispatch().copy()}
    want_guard_hits = o.guard_hits()
L.ribbit_debug_set_merge_min_range(5)
def check(got):
    for k, w in want.items():
        assert np.array_equal(got[k].view("<i4"), w.view("<i4")), k
    assert got["guard_hits"] == want_guard_hits
    merged = (C.c_int32 * 5)()
    L.ribbit_debug_last_merge(1, C.byref(merged))
    assert merged[0] >= 2, merged[0]           # the anchored stage ran in ranges, not in call order on one thread
exercise(lambda: ribbit_amd.host_replay_calls(m_lo, m_hi, seq, *calls), check)
""",
    # a piece per 1024 seeds (api_align.cpp); the longest run of ones of the oracle's composed plane over every interval
    "longest_runs": ORACLE_CASE + r"""
with Oracle(seq, m_lo, m_hi) as o:
    o.run_perfect(); o.run_subst(); o.run_anchor_planes()
    planes = {m: o.plane(m).astype(np.int8) for m in range(m_lo, m_hi + 1)}
rs = np.random.RandomState(11)
n = 3 * 1024 + 77
ms = rs.randint(m_lo, m_hi + 1, n)
a = rs.randint(0, len(seq) - 1, n)
b = np.minimum(len(seq), a + 1 + rs.randint(0, 6 * ms + 64))
seeds = np.zeros(n, ribbit_amd.SEED_DT)
seeds["start"], seeds["end"], seeds["mlen"] = a, b, ms
def longest(bits):
    edge = np.diff(np.concatenate(([0], bits, [0])))
    runs = np.flatnonzero(edge == -1) - np.flatnonzero(edge == 1)
    return int(runs.max()) if len(runs) else 0
want = [longest(planes[int(m)][int(s):int(e)]) for s, e, m in zip(a, b, ms)]
assert max(want) >= 8
def check(got):
    assert got.tolist() == want
exercise(lambda: ribbit_amd.host_longest_runs(m_lo, m_hi, seq, seeds), check)
""",
    # 17 MB of rows: four pieces of whole lines (api_mask.cpp)
    "bed_intervals": r"""
rs = np.random.RandomState(5)
n = 330_000
starts = rs.randint(0, 1 << 30, n)
ends = starts + rs.randint(-5, 120_000, n)
text = "".join(f"chr\t{s}\t{e}\tACG\t3 | 3\t{e - s}\t4\t0.9\t+\tSEED-5\t12=3=7=\n" for s, e in zip(starts.tolist(), ends.tolist())).encode()
assert len(text) >= 17 << 20
def check(got):
    assert got.shape == (n, 2) and (got[:, 0] == starts).all() and (got[:, 1] == ends).all()
exercise(lambda: ribbit_amd.bed_intervals(text), check)
""",
    # 17 MB of rows, every row a locus of its own: the line starts in four pieces, the 330,000 loci's lines in as many (api_loci.cpp)
    "bed_loci_text": r"""
import loci_contract
rs = np.random.RandomState(6)
n = 330_000
starts = np.arange(n, dtype=np.int64) * 3000 + rs.randint(0, 1000, n)
ends = starts + rs.randint(1, 1900, n)
order = rs.permutation(n)                      # row order of the text; the loci are by ascending start
bed = "".join(f"chr\t{starts[i]}\t{ends[i]}\tACGT\t4 | 4\t{ends[i] - starts[i]}\t4\t0.9\t+\tSEED-5\t12=3=7=\n" for i in order.tolist())
assert len(bed) >= 17 << 20 and n >= 8192
line_of = np.empty(n, np.int64)
line_of[order] = np.arange(n)
loci = np.zeros(n, ribbit_amd.LOCUS_DT)
loci["start"], loci["end"], loci["rows"], loci["covered"], loci["best_row"] = starts, ends, 1, ends - starts, line_of
want = loci_contract.loci_lines("chr7", bed, loci.tolist()).encode()
raw = bed.encode()
def check(got):
    assert got == want
exercise(lambda: ribbit_amd.bed_loci_text("chr7", raw, loci), check)
""",
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_refused_thread_changes_nothing_and_a_throwing_part_is_nomem(case):
    env = {k: v for k, v in os.environ.items() if k != "RIBBIT_HIP_LIBRARY"}      # the ordinary library
    env["RIBBIT_THREADS"] = "4"
    out = subprocess.run([sys.executable, "-c", PROLOGUE % {"root": ROOT} + CASES[case]], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"child exit status {out.returncode}\n{out.stdout[-1000:]}\n{out.stderr[-3000:]}"
    for line in ("refused-start-0-same-result", "refused-start-1-same-result", "thrown-in-part-0-nomem-then-right", "thrown-in-part-1-nomem-then-right"):
        assert line in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
