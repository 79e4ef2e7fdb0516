"""GPU checks of the anchored merge kernel (anchored_merge.hip) range by range, on the constructed cases of tests/merge_contract.py
through ribbit_hip_debug_merge_ranges: the lanes alone, no host thread beside them.  Every range on its own (only_range) leaves
exactly what a host worker leaves for it -- status, own list, guard count, cursors, by-counter read masks, and the undo, foreign-read
and head-write logs as sorted sets -- and what pyref leaves; its status is the one predicted from pyref's sizes and the reported
caps, so no range bails unpredicted; every tag of the contract is reached by a range that a lane merged with status 0.  All ranges
in one launch, with one, two and the default number of resident wavefronts (lanes then take several ranges, also after one that
bailed), give the lists and guards of pyref and of the host, and the device count is the number of ranges predicted to fit.
Budgets: a pass budget that only the heavy ranges exceed, logs too small, a device limit.  Bit-exact: no tolerances."""
import pytest

import merge_contract as mc
import ribbit_amd
from test_merge_ranges import CASES, heads_without_flag, host_raw, reference, run, seeds, tags_of

pytestmark = pytest.mark.gpu
LANES, HOST = ribbit_amd.MERGE_ON_LANES, ribbit_amd.MERGE_ON_HOST

@pytest.fixture(scope="module")
def scanner():
    with ribbit_amd.Scanner(2, 100) as sc:
        yield sc


@pytest.fixture(scope="module")
def alone(scanner):
    """case -> (the raw result of every range run on the lanes on its own, the tags of those a lane merged with status 0);
    computed once per case, whichever test asks first"""
    done = {}

    def of(case):
        if case.name not in done:
            nr = len(host_raw(case)["cuts"])
            runs = [run(case, scanner, where=LANES, only_range=k, max_passes=1 << 20) for k in range(nr)]
            met = set()
            for k, dev in enumerate(runs):
                if dev["ran"] and dev["ranges"][k]["status"] == 0:
                    met |= tags_of(case, k, dev["ranges"])
            done[case.name] = (runs, met)
        return done[case.name]
    return of


def predicted(case, k):
    return mc.predicted_status(reference(case, k)["peaks"], host_raw(case)["caps"])


def same_as_reference(got, case, k):
    ref = reference(case, k)
    assert (seeds(got["own"]), got["guard_hits"], got["cursor"], got["undo"], heads_without_flag(got)) == \
           (ref["own"], ref["guards"], ref["cursor"], ref["undo"], ref["heads"]), (case.name, k)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_range_on_its_own_equals_the_host_worker_and_pyref(alone, case):
    prep = host_raw(case)
    nr = len(prep["cuts"])
    runs, met = alone(case)
    for k in range(nr):
        dev = runs[k]
        assert dev["ran"] and list(dev["cuts"]) == list(prep["cuts"]) and list(dev["first"]) == list(prep["first"])
        assert dev["cursors0"].tolist() == prep["cursors0"].tolist()
        assert [i for i, r in enumerate(dev["ranges"]) if r["status"] != 0xFFFFFFFF] == [k]
        got = dev["ranges"][k]
        assert got["status"] == predicted(case, k), (case.name, k, reference(case, k)["peaks"])
        if got["status"]:
            continue
        host = run(case, where=HOST, only_range=k)["ranges"][k]
        for key in ("status", "guard_hits", "cursor", "head_reads", "undo", "reads", "heads"):
            assert got[key] == host[key], (case.name, k, key)
        assert seeds(got["own"]) == seeds(host["own"]), (case.name, k)
        same_as_reference(got, case, k)
    # every path the case exists for was reached in a range that a lane merged
    assert [t for t in case.tags if t not in met] == []


def test_every_tag_of_the_contract_is_met_by_a_range_a_lane_merged(alone):
    met = set().union(*(alone(case)[1] for case in CASES))
    assert [t for t in mc.all_tags() if t not in met] == []


def test_a_stride_larger_than_the_words_used_on_the_lanes(scanner):
    """(e) the planes with 37 words more to a row than the record needs, the extra words all ones: a lane that worked the stride out
    of the length, or read past a row's used words, would count other bits.  Every range on its own equals the host worker (same
    wide planes) and pyref; the whole stage equals pyref."""
    import numpy as np
    case = [c for c in CASES if c.name == "plane reads"][0]
    xa, stride = ribbit_amd.pack_bit_planes([case.planes[m] for m in range(case.m_lo, case.m_hi + 1)], case.length)
    wide = np.full((xa.shape[0], stride + 37), 0xFFFFFFFF, dtype="<u4")
    wide[:, :stride] = xa
    args = (case.m_lo, case.m_hi, case.length, case.perfect, case.subst, case.calls, wide, stride + 37)
    nr = len(host_raw(case)["cuts"])
    nested = 0
    for k in range(nr):
        got = ribbit_amd.debug_merge_ranges(scanner, *args, where=LANES, only_range=k)["ranges"][k]
        host = ribbit_amd.debug_merge_ranges(None, *args, where=HOST, only_range=k)["ranges"][k]
        assert got["status"] == 0
        for key in ("guard_hits", "cursor", "head_reads", "undo", "reads", "heads"):
            assert got[key] == host[key], (k, key)
        assert seeds(got["own"]) == seeds(host["own"]), k
        same_as_reference(got, case, k)
        nested += any(t.startswith("plane read") for t, n in reference(case, k)["met"].items() if n)
    assert nested >= 16
    full = ribbit_amd.debug_merge_ranges(scanner, *args, where=LANES, full=True)
    p, s, a, guards = mc.ref_full(case)
    assert (seeds(full["lists"]["anchored"]), full["lists"]["guard_hits"], full["device_merge"][0]) == (a, guards, nr)


@pytest.mark.parametrize("waves", [1, 2, 0])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_all_ranges_in_one_launch_lanes_alone(scanner, case, waves):
    prep = host_raw(case)
    nr = len(prep["cuts"])
    fits = sum(1 for k in range(nr) if predicted(case, k) == 0)
    full = run(case, scanner, where=LANES, full=True, resident_waves=waves, max_passes=1 << 20)
    host = run(case, where=HOST, full=True)
    p, s, a, guards = mc.ref_full(case)
    for lists in (full["lists"], host["lists"]):
        assert (seeds(lists["perfect"]), seeds(lists["subst"]), seeds(lists["anchored"]), lists["guard_hits"]) == (p, s, a, guards)
    assert full["ran"]
    assert full["device_merge"][:4] == (fits, nr - fits, 0, nr)
    # raw, all ranges in one launch, whichever lane took a range after whichever other: a range that read no seed left of itself
    # leaves what it leaves on its own
    raw = run(case, scanner, where=LANES, resident_waves=waves, max_passes=1 << 20)
    for k in range(nr):
        got = raw["ranges"][k]
        assert got["status"] == predicted(case, k), (case.name, k)
        if not got["status"] and not prep["ranges"][k]["reads"]:
            assert got["reads"] == []
            same_as_reference(got, case, k)


def test_lanes_take_a_range_after_one_that_bailed(scanner):
    """64 lanes, more ranges than that, and ranges that overflow among them: a lane goes on with another range after each"""
    both = mc.lanes_case()
    nr = len(host_raw(both)["cuts"])
    assert nr >= 130
    status = [predicted(both, k) for k in range(nr)]
    assert any(status[:64]) and any(status[64:]) and not all(status)
    raw = run(both, scanner, where=LANES, resident_waves=1, max_passes=1 << 20)
    for k in range(nr):
        assert raw["ranges"][k]["status"] == status[k], k
        if not status[k]:
            same_as_reference(raw["ranges"][k], both, k)


def test_a_lane_that_gave_a_range_up_merges_the_next_one(scanner):
    """The lanes take the ranges in the order of the work the calls promise, and every range here is one call: in index order, 64 at
    a time.  A dense range keeps its lane for a few hundred passes, by which time the other lanes have emptied the list; so the
    budget of passes is set to 24, which a lone call with four candidates at most stays far below (a dozen passes: see the test
    below) and a dense range exceeds at once.  Its lane then takes one of the 180 ranges still waiting, and must merge it as any
    other lane would: status, retirements and guards start afresh."""
    case = mc.caps_case(repeats=6, name="lanes, six times")[0]
    prep = run(case, where=HOST)
    nr = len(prep["cuts"])
    assert nr >= 250
    raw = run(case, scanner, where=LANES, resident_waves=1, max_passes=24)
    gave_up = merged = 0
    for k in range(nr):
        ref, got = mc.ref_range(case, prep, k), raw["ranges"][k]
        if ref["peaks"]["cands"] > 24:
            gave_up += 1
            assert got["status"] not in (0, 0xFFFFFFFF), k
        elif ref["peaks"]["cands"] <= 4:
            merged += 1
            assert got["status"] == 0, k
            assert (seeds(got["own"]), got["guard_hits"], got["cursor"], got["undo"]) == (ref["own"], ref["guards"], ref["cursor"], ref["undo"]), k
    assert gave_up >= 60 and merged >= 120


def test_a_pass_budget_only_the_heavy_ranges_exceed(scanner):
    """A lane judges one candidate per pass of its loop, so a call with more candidates than the budget cannot fit it: every such
    range reports `too_slow` (or the overflow predicted for it, whichever its lane meets first).  A lone call with four candidates
    at most needs one pass to take the range, one to fetch the call, one per cursor step (the start cursors are already in place:
    a handful), one per four entries of the first walk, one per candidate and one for the tail: far below 64.  Those ranges, in
    the same wavefront as the heavy ones, are merged and leave exactly what they leave without a budget."""
    case = [c for c in CASES if c.name == "caps"][0]
    nr = len(host_raw(case)["cuts"])
    budget = 64
    raw = run(case, scanner, where=LANES, max_passes=budget)
    caps = raw["caps"]
    heavy = light = 0
    for k in range(nr):
        ref, got = reference(case, k), raw["ranges"][k]
        assert got["status"] != 0xFFFFFFFF
        if ref["peaks"]["cands"] > budget:
            heavy += 1
            assert got["status"] and got["status"] & (caps["too_slow"] | predicted(case, k)) == got["status"], k
        elif ref["peaks"]["cands"] <= 4:
            light += 1
            host = run(case, where=HOST, only_range=k)["ranges"][k]
            assert got["status"] == 0, k
            same_as_reference(got, case, k)
            assert (got["head_reads"], got["reads"], got["heads"]) == (host["head_reads"], host["reads"], host["heads"]), k
        else:
            assert got["status"] in (0, caps["too_slow"]), k
            if not got["status"]:
                same_as_reference(got, case, k)
    assert heavy >= 6 and light >= 10


def test_logs_too_small_and_a_device_limit(scanner):
    logged = lambda c: sum(len(r["undo"]) + len(r["reads"]) for r in host_raw(c)["ranges"])
    case = [c for c in CASES if logged(c) >= 2][0]
    nr = len(host_raw(case)["cuts"])
    small = run(case, scanner, where=LANES, log_cap=1, max_passes=1 << 20)
    ok = run(case, scanner, where=LANES, max_passes=1 << 20)
    n_log = sum(len(r["undo"]) + len(r["reads"]) for r in ok["ranges"])
    assert n_log >= 2 and not small["ran"] and small["ranges"] == []
    # ... and the stage then runs on the host, with the same lists
    full = run(case, scanner, where=LANES, full=True, log_cap=1, max_passes=1 << 20)
    p, s, a, guards = mc.ref_full(case)
    assert (seeds(full["lists"]["perfect"]), seeds(full["lists"]["subst"]), seeds(full["lists"]["anchored"]), full["lists"]["guard_hits"]) == (p, s, a, guards)
    assert full["device_merge"][:3] == (0, 0, 0)
    limited = run(case, scanner, where=LANES, device_limit=2, max_passes=1 << 20)
    taken = [k for k, r in enumerate(limited["ranges"]) if r["status"] != 0xFFFFFFFF]
    assert len(taken) == 2 and all(limited["ranges"][k]["status"] == predicted(case, k) for k in taken)
    # the log of the writes to list heads
    heads = [c for c in CASES if c.name == "list heads"][0]
    assert sum(len(r["heads"]) for r in run(heads, scanner, where=LANES)["ranges"]) >= 2
    small = run(heads, scanner, where=LANES, head_cap=1)
    assert not small["ran"] and small["ranges"] == []
    full = run(heads, scanner, where=LANES, full=True, head_cap=1)
    assert (seeds(full["lists"]["anchored"]), full["device_merge"][:3]) == (mc.ref_full(heads)[2], (0, 0, 0))


@pytest.mark.parametrize("calls_per_range", [1, 8])
def test_fuzz_records_lanes_alone(calls_per_range):
    """the fuzz records of tests/test_device_merge_gpu.py through the entry point: their own lists, planes and anchored calls, the
    lanes alone.  The stage's lists equal the oracle's, and the device merged every range that pyref (one run in call order, its
    peaks per call) shows to stay clear of the caps -- no range bails unpredicted.  The budget of passes is lifted: with the
    production budget one range of 541 calls on one another (seed 7) is `too_slow`, as meant, and the host's."""
    import numpy as np

    import pyref
    from fuzz import fuzz_case
    from oracle_lib import LIST_ANCHORED, LIST_PERFECT, LIST_SUBST, Oracle
    ranges = merged = 0
    for seed in range(60):
        seq, m_lo, m_hi = fuzz_case(41000 + seed, scale=3)
        if len(seq) < 64:
            continue
        with ribbit_amd.Scanner(m_lo, m_hi) as sc, Oracle(seq, m_lo, m_hi) as o:
            sc.load_record(seq)
            calls = sc.anchored_calls()
            perfect, subst = sc.processShiftXORswithSubstitutions()
            stride = len(seq) // 32 + 1
            xa = sc.xa_words(0, stride)
            args = (sc, m_lo, m_hi, len(seq), perfect, subst, calls, xa, stride)
            try:
                full = ribbit_amd.debug_merge_ranges(*args, where=LANES, full=True, calls_per_range=calls_per_range, max_passes=1 << 20)
            except ribbit_amd.RibbitHipError as e:
                assert "two ranges" in str(e), (seed, e)          # (too few calls to cut)
                continue
            o.run_all()
            lists = full["lists"]
            for mine, theirs in ((lists["perfect"], o.seeds(LIST_PERFECT)), (lists["subst"], o.seeds(LIST_SUBST)), (lists["anchored"], o.seeds(LIST_ANCHORED))):
                assert np.array_equal(mine.view("<i4"), theirs.view("<i4")), seed
            assert lists["guard_hits"] == o.guard_hits(), seed
            # which ranges fit: pyref's peaks per call, far enough from every cap that a neighbour's retirement cannot matter
            bits = np.unpackbits(xa.view(np.uint8), axis=1, bitorder="little")[:, :len(seq)]
            am = pyref.AnchoredMerge(perfect.tolist(), subst.tolist(), {m: bits[m - m_lo] for m in range(m_lo, m_hi + 1)}, len(seq))
            am.run([tuple(int(v) for v in c) for c in calls.tolist()])
            kept = [i for i, c in enumerate(calls.tolist()) if c[0] != len(seq) and c[3] - c[2] >= pyref.anchored_cutoff(c[1])]
            caps, first = full["caps"], full["first"]
            assert first[-1] == len(kept), seed
            clear = 0
            for k in range(len(full["cuts"])):
                peaks = [am.peaks[kept[i]] for i in range(first[k], first[k + 1])]
                top = {key: max(p[key] for p in peaks) + 2 for key in ("ps", "cands", "factor", "nonfactor", "sizes")}
                clear += mc.predicted_status(top, caps) == 0
            assert full["ran"] and full["device_merge"][0] >= clear and sum(full["device_merge"][:2]) == full["device_merge"][3] == len(full["cuts"]), (seed, full["device_merge"], clear)
            ranges += len(full["cuts"])
            merged += full["device_merge"][0]
    assert ranges > 200 and merged * 100 >= ranges * 95, (ranges, merged)
