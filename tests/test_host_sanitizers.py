"""The host half of the product (seed merges, window state machines, refinement, own Smith-Waterman, BED writer) under
AddressSanitizer + UBSan: `make -C ribbit_amd/csrc asan` builds the library with its HOST code instrumented, and a
child interpreter replays oracle call logs through the host-only entry points on adversarial records, including the
motif sizes above 192 bases whose atomicity test once read out of bounds.  (GPU sanitizers are not available on the
pool; the kernels are covered by the parity tests.)"""
import glob
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_SO = os.path.join(ROOT, "ribbit_amd", "libribbit_hip_asan.so")

CHILD = r"""
import sys
sys.path[:0] = [%(tests)r, %(root)r]
import numpy as np
import ribbit_amd
from fuzz import fuzz_case
from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle
cases = [(s, 1) for s in range(9000, 9040)] + [(82531, 16), (86001, 16), (86007, 16)]
for seed, scale in cases:
    seq, m_lo, m_hi = fuzz_case(seed, scale)
    with Oracle(seq, m_lo, m_hi) as o:
        o.run_perfect(); pc = o.calls(LIST_PERFECT)
        o.run_subst(); sc = o.calls(LIST_SUBST)
        o.run_anchor_planes()
        xa, stride = ribbit_amd.pack_bit_planes([o.plane(m) for m in range(m_lo, m_hi + 1)], len(seq))
        o.run_anchored(); o.run_dispatch()
        r = ribbit_amd.host_replay_calls(m_lo, m_hi, seq, pc, sc, o.calls(LIST_ANCHORED), xa, stride)
        assert np.array_equal(r["dispatch"].view("<i4"), o.dispatch().view("<i4")), seed
        if len(seq):
            ribbit_amd.host_refine_jobs(m_lo, m_hi, seq, xa, stride, o.dispatch())
            assert ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, o.dispatch(), "fz") == o.refine_bed("fz"), seed
print("host-sanitizer-run-ok")
"""


def test_host_code_clean_under_sanitizers():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ribbit_amd", "csrc"), "asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and os.path.exists(ASAN_SO), r.stderr[-3000:]
    rts = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.asan-x86_64.so")
    if not rts:
        pytest.skip("clang's shared ASan runtime not found")
    env = dict(os.environ, LD_PRELOAD=rts[0], RIBBIT_HIP_LIBRARY=ASAN_SO, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([sys.executable, "-c", CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT}], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "host-sanitizer-run-ok" in out.stdout, out.stderr[-4000:]


TSAN_SO = os.path.join(ROOT, "ribbit_amd", "libribbit_hip_tsan.so")

TSAN_CHILD = r"""
import os, sys
sys.path[:0] = [%(tests)r, %(root)r]
import numpy as np
import ribbit_amd
from fuzz import fuzz_case
from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle
from ribbit_amd.simulate import simulate_sequence
lib = ribbit_amd.load_library()
# seed 38 at 300 kb: the record whose one list-head write (Q8) changes its entry -- logged by a worker, decided after the pass
cases = [fuzz_case(s) for s in range(9000, 9010)] + [(simulate_sequence(300_000, 38, 2, 30)[0], 2, 30),
                                                      (simulate_sequence(200_000, 17, 2, 60, n_block_rate=0.3)[0], 2, 60)]
faults = 0
for min_range in (1, 16):
    lib.ribbit_debug_set_merge_min_range(min_range)
    for seq, m_lo, m_hi in cases:
        with Oracle(seq, m_lo, m_hi) as o:
            o.run_perfect(); pc = o.calls(LIST_PERFECT)
            o.run_subst(); sc = o.calls(LIST_SUBST)
            o.run_anchor_planes()
            xa, stride = ribbit_amd.pack_bit_planes([o.plane(m) for m in range(m_lo, m_hi + 1)], len(seq))
            o.run_anchored(); o.run_dispatch()
            r = ribbit_amd.host_replay_calls(m_lo, m_hi, seq, pc, sc, o.calls(LIST_ANCHORED), xa, stride)
            assert np.array_equal(r["anchored"].view("<i4"), o.seeds(LIST_ANCHORED).view("<i4"))
            assert np.array_equal(r["dispatch"].view("<i4"), o.dispatch().view("<i4"))
            # the ranges of the GPU's pass of the anchored merge with a device that cannot run (parallel_merge.h: AnchoredDevicePass):
            # cuts searched in pieces, cursors by bisection, host threads taking ranges from the back of a list the "lanes" take from the front
            os.environ["RIBBIT_MERGE_DEVICE_RANGES"] = "4"
            r = ribbit_amd.host_replay_calls(m_lo, m_hi, seq, pc, sc, o.calls(LIST_ANCHORED), xa, stride)
            del os.environ["RIBBIT_MERGE_DEVICE_RANGES"]
            assert np.array_equal(r["anchored"].view("<i4"), o.seeds(LIST_ANCHORED).view("<i4"))
            if len(seq) and min_range == 16:
                os.environ["RIBBIT_DEBUG_JOB_SLICES"] = "3"          # the refinement pipeline's slice builder (one parallel region)
                ribbit_amd.host_refine_jobs(m_lo, m_hi, seq, xa, stride, o.dispatch())
                del os.environ["RIBBIT_DEBUG_JOB_SLICES"]
                assert ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, o.dispatch(), "fz") == o.refine_bed("fz")
                # the recursion cut into nodes, pieces and levels (refine.h: DeferredNode): writers on several threads hand their
                # nodes to one list and their pieces to another
                os.environ["RIBBIT_HOST_DEFER"] = "1"; os.environ["RIBBIT_DEFER_MIN"] = "30"
                assert ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, o.dispatch(), "fz") == o.refine_bed("fz")
                del os.environ["RIBBIT_HOST_DEFER"], os.environ["RIBBIT_DEFER_MIN"]
                # the teams' helper with its faults injected (host_threads.h): a thread that does not start leaves its part to the
                # caller; a part that throws hands its exception to the caller behind the joins
                lib.ribbit_host_debug_thread_faults(1, -1)
                assert ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, o.dispatch(), "fz") == o.refine_bed("fz")
                faults += lib.ribbit_host_debug_thread_faults(-1, 1)
                for call in (lambda: ribbit_amd.host_replay_calls(m_lo, m_hi, seq, pc, sc, o.calls(LIST_ANCHORED), xa, stride),
                             lambda: ribbit_amd.host_refine_bed(m_lo, m_hi, seq, xa, stride, o.dispatch(), "fz")):
                    try:
                        call()
                        raised = False
                    except ribbit_amd.RibbitHipError as e:
                        assert "out of host memory" in str(e)
                        raised = True
                    fired = lib.ribbit_host_debug_thread_faults(-1, 1)          # (of this call; the mode stays)
                    assert raised == (fired > 0), (raised, fired)             # a team formed and its part threw: the call says so
                    faults += fired
                lib.ribbit_host_debug_thread_faults(-1, -1)
assert faults > 0
print("host-tsan-run-ok")
"""


def test_host_threads_clean_under_thread_sanitizer():
    """The range-parallel merges (workers that log Q8's list-head writes and the types they read, the validation walk behind
    them), the slice builder of the refinement pipeline and the refinement threads, without a GPU, under ThreadSanitizer
    (`make tsan`).  Round 4's first run of it found three formal races -- plain reads of a seed's type beside another range's
    atomic retirement of it (seed_lists.cpp: the validation pass makes the outcome right either way, but a plain read racing
    an atomic store is still undefined behaviour) -- now relaxed atomic loads; the run must stay free of reports."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "ribbit_amd", "csrc"), "tsan", "-j4"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and os.path.exists(TSAN_SO), r.stderr[-3000:]
    rts = glob.glob("/opt/rocm/lib/llvm/lib/clang/*/lib/linux/libclang_rt.tsan-x86_64.so")
    if not rts:
        pytest.skip("clang's shared TSan runtime not found")
    env = dict(os.environ, LD_PRELOAD=rts[0], RIBBIT_HIP_LIBRARY=TSAN_SO, RIBBIT_THREADS="8",
               TSAN_OPTIONS="halt_on_error=0:report_signal_unsafe=0:history_size=4:exitcode=66")
    out = subprocess.run([sys.executable, "-c", TSAN_CHILD % {"tests": os.path.join(ROOT, "tests"), "root": ROOT}], env=env,
                         capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "host-tsan-run-ok" in out.stdout and "ThreadSanitizer" not in out.stderr, out.stderr[-6000:]
