"""No entry point lets a C++ exception out of the library (include/ribbit_hip.h, api_internal.h: guarded): a host allocation
that fails is RIBBIT_E_NOMEM and a message, not the end of the calling process.

Each case runs in a child interpreter, so that a regression shows as the child's exit status (134: terminate called after
throwing an instance of 'std::bad_alloc') and not as the death of pytest.  The sizes are far beyond the address space
(2^45 parts of 99 motif sizes and 8 bytes: 2.8e16 bytes; 2^50 plane words: 4.5e15 bytes a plane), so the allocation is
refused on any machine whatever its overcommit setting, and every case reaches it before the library reads any caller memory
of that size: the arrays passed are null or tiny.  Host-only entry points: no GPU.  Not run against the sanitizer builds,
whose allocator reports oversized requests in its own way."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROLOGUE = r"""
import ctypes as C, sys
sys.path[:0] = [%(root)r]
import ribbit_amd
L = ribbit_amd.load_library()
params = ribbit_amd.ScanParams()
L.ribbit_scan_params_default(C.byref(params), 2, 100)
E_NOMEM = -4
def check(rc):
    msg = L.ribbit_hip_last_error().decode()
    assert rc == E_NOMEM, (rc, msg)
    assert "out of host memory" in msg, msg
    print("returned-nomem")
"""

CASES = {
    # std::vector<rb::Seg>(nm * nparts) before the first read of events / counts
    "perfect_runs_from_events": r"""
counts = (C.c_uint64 * 99)()
runs, n = C.c_void_p(), C.c_size_t()
check(L.ribbit_host_perfect_runs_from_events(C.byref(params), 1 << 45, None, C.addressof(counts), C.byref(runs), C.byref(n)))
""",
    # HostPlanes::resize(length, nwords) before the planes are copied; an empty record's planes may be null
    "longest_runs": r"""
check(L.ribbit_host_longest_runs(C.byref(params), 0, None, None, None, 1 << 50, None, 0, None))
""",
    "replay_calls": r"""
out = ribbit_amd.SeedLists()
check(L.ribbit_host_replay_calls(C.byref(params), 0, None, None, None, 1 << 50, None, 0, None, 0, None, 0, None, 0, C.byref(out)))
assert not out.perfect and not out.dispatch
""",
    # the same through the entry point that had a handler for std::bad_alloc before: its message is unchanged
    "merge_chunks": r"""
out = ribbit_amd.SeedLists()
rc = L.ribbit_host_merge_chunks(C.byref(params), 0, None, None, None, 1 << 50, None, 0, None, 0, C.byref(out))
assert L.ribbit_hip_last_error().decode() == "out of host memory in the merge of the chunks"
check(rc)
assert not out.perfect and not out.dispatch
""",
    # ribbit_hip_debug_merge_ranges: null arguments and knobs out of range are RIBBIT_E_ARG before anything is read; the copy of the
    # planes (2^40 words a plane) is refused as out of memory, not thrown through the C boundary
    "debug_merge_ranges": r"""
knobs, out = ribbit_amd.DebugMergeKnobs(1, 0, 1, 0, 0, 0, 0, -1, -1), ribbit_amd.DebugMergeRanges()
word = (C.c_uint32 * 4)()
E_ARG = -1
call = L.ribbit_hip_debug_merge_ranges
assert call(None, None, 100, None, 0, None, 0, None, 0, C.addressof(word), 4, C.byref(knobs), C.byref(out)) == E_ARG
assert call(None, C.byref(params), 100, None, 0, None, 0, None, 0, None, 4, C.byref(knobs), C.byref(out)) == E_ARG
assert call(None, C.byref(params), 100, None, 0, None, 0, None, 0, C.addressof(word), 4, None, C.byref(out)) == E_ARG
assert call(None, C.byref(params), 100, None, 0, None, 0, None, 0, C.addressof(word), 4, C.byref(knobs), None) == E_ARG
assert call(None, C.byref(params), 100, None, 1, None, 0, None, 0, C.addressof(word), 4, C.byref(knobs), C.byref(out)) == E_ARG
for field, value in (("where", 2), ("calls_per_range", 0), ("resident_waves", -1), ("max_passes", -1), ("head_cap", -1), ("log_cap", -1), ("only_range", -2)):
    bad = ribbit_amd.DebugMergeKnobs(1, 0, 1, 0, 0, 0, 0, -1, -1)
    setattr(bad, field, value)
    assert call(None, C.byref(params), 100, None, 0, None, 0, None, 0, C.addressof(word), 4, C.byref(bad), C.byref(out)) == E_ARG, field
L.ribbit_debug_merge_ranges_free(None)
check(call(None, C.byref(params), 100, None, 0, None, 0, None, 0, C.addressof(word), 1 << 40, C.byref(knobs), C.byref(out)))
assert not out.cuts and not out.own
""",
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_unallocatable_size_is_nomem_not_the_end_of_the_process(case):
    env = {k: v for k, v in os.environ.items() if k != "RIBBIT_HIP_LIBRARY"}      # the ordinary library
    out = subprocess.run([sys.executable, "-c", PROLOGUE % {"root": ROOT} + CASES[case]], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"child exit status {out.returncode}\n{out.stderr[-3000:]}"
    assert "returned-nomem" in out.stdout, out.stdout[-1000:] + out.stderr[-3000:]
