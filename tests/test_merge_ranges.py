"""CPU checks of tests/merge_contract.py and of the host workers behind ribbit_hip_debug_merge_ranges: for every constructed case
pyref reaches the paths the case names; every range the host workers merge on its own leaves what pyref leaves (own list, guard
count, cursors, retirements); the whole stage through the entry point equals pyref in call order and ribbit_host_replay_calls.
No GPU: the entry point takes a null handle for the host workers.  Everything is integers: equality throughout."""
import functools

import numpy as np
import pytest

import merge_contract as mc
import ribbit_amd

CASES = mc.all_cases()


def run(case, scanner=None, **knobs):
    xa, stride = packed(case)
    knobs.setdefault("calls_per_range", case.calls_per_range)
    return ribbit_amd.debug_merge_ranges(scanner, case.m_lo, case.m_hi, case.length, case.perfect, case.subst, case.calls, xa, stride, **knobs)


@functools.lru_cache(maxsize=None)
def packed(case):
    return ribbit_amd.pack_bit_planes([case.planes[m] for m in range(case.m_lo, case.m_hi + 1)], case.length)


@functools.lru_cache(maxsize=None)
def host_raw(case):
    return run(case, where=ribbit_amd.MERGE_ON_HOST)


@functools.lru_cache(maxsize=None)
def reference(case, k):
    return mc.ref_range(case, host_raw(case), k)


def tags_of(case, k, ranges):
    """the paths range k took: pyref's tags, and what the logged head writes of the run say about their targets"""
    return {t for t, n in reference(case, k)["met"].items() if n} | {f"head write changed_then {w[6]}" for w in ranges[k]["heads"]}


def heads_without_flag(r):
    return sorted(w[:6] for w in r["heads"])


def seeds(a):
    return [tuple(int(v) for v in s) for s in a.tolist()]


def test_the_library_reports_its_caps():
    caps = host_raw(CASES[0])["caps"]
    assert caps == mc.library_caps() and all(caps[k] > 0 for k in ribbit_amd.MERGE_CAPS)
    assert caps["ps_cap"] < caps["cand_cap"] and len({caps[k] for k in ("scratch_full", "log_full", "bad_plane", "runaway", "too_slow")}) == 5


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_pyref_meets_the_tags_of_the_case_in_ranges_predicted_to_fit(case):
    raw = host_raw(case)
    assert len(raw["cuts"]) >= 2
    met = set()
    for k in range(len(raw["cuts"])):
        ref = reference(case, k)
        if mc.predicted_status(ref["peaks"], raw["caps"]) == 0:
            met |= tags_of(case, k, raw["ranges"])
    assert [t for t in case.tags if t not in met] == []


def test_every_tag_of_the_contract_is_met_by_some_case_in_a_range_predicted_to_fit():
    met = set()
    for case in CASES:
        raw = host_raw(case)
        for k in range(len(raw["cuts"])):
            if mc.predicted_status(reference(case, k)["peaks"], raw["caps"]) == 0:
                met |= tags_of(case, k, raw["ranges"])
    assert len(mc.REQUIRED_TAGS) > 100 and set(mc.REQUIRED_TAGS) <= set(mc.all_tags())
    assert [t for t in mc.all_tags() if t not in met] == []


def test_the_cap_case_stands_at_every_cap():
    case, wanted = mc.caps_case()
    raw = host_raw(CASES[[c.name for c in CASES].index("caps")])
    peaks = [reference(CASES[[c.name for c in CASES].index("caps")], k)["peaks"] for k in range(len(raw["cuts"]))]
    key, caps0 = {"ps": "ps", "factor": "factor", "nonfactor": "nonfactor"}, raw["caps"]
    for kind, n in wanted:
        assert any(p[key[kind]] == n for p in peaks), (kind, n)
    caps = raw["caps"]
    # the perfect-plus-substitution candidates are all the candidates there; the factor coverage table holds a key per child
    for n in (caps["cand_cap"], caps["cand_cap"] + 1):
        assert any(p["cands"] == n for p in peaks), n
    for n in (caps["cov_cap"] - 1, caps["cov_cap"], caps["cov_cap"] + 1):
        assert any(p["sizes"] == n for p in peaks), n
    status = [mc.predicted_status(p, caps) for p in peaks]
    assert 0 < sum(1 for s in status if s) < len(status) / 3
    # the far end of the candidate spill, the perfect-plus-substitution candidates inside theirs
    spill = CASES[[c.name for c in CASES].index("cand spill end")]
    peaks = [reference(spill, k)["peaks"] for k in range(len(host_raw(spill)["cuts"]))]
    end = caps["cand_cap"] + caps["cand_spill"]
    for n in (end - 1, end, end + 1):
        assert any(p["cands"] == n and p["ps"] <= caps["ps_cap"] + caps["ps_spill"] for p in peaks), n
    assert sorted(mc.predicted_status(p, caps) for p in peaks if p["cands"] >= end - 1)[:3] == [0, 0, caps["scratch_full"]]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_workers_leave_what_pyref_leaves_range_by_range(case):
    raw = host_raw(case)
    nr = len(raw["cuts"])
    kept, _ = case.kept()
    assert raw["ran"] and len(raw["ranges"]) == nr and raw["first"][0] == 0 and raw["first"][-1] == len(kept)
    assert list(raw["cuts"][1:]) == sorted(raw["cuts"][1:]) and all(a < b for a, b in zip(raw["first"], raw["first"][1:]))
    for k in range(nr):
        got, ref = raw["ranges"][k], reference(case, k)
        alone = run(case, where=ribbit_amd.MERGE_ON_HOST, only_range=k)["ranges"]
        assert [r["status"] for i, r in enumerate(alone) if i != k] == [0xFFFFFFFF] * (nr - 1)
        # (the run of all ranges at once only where the range read no seed left of itself: a neighbour may retire such a seed meanwhile)
        for r in (got, alone[k]) if not got["reads"] else (alone[k],):
            assert r["status"] == 0
            assert seeds(r["own"]) == ref["own"], (case.name, k)
            assert (r["guard_hits"], r["cursor"], r["undo"], heads_without_flag(r)) == (ref["guards"], ref["cursor"], ref["undo"], ref["heads"]), (case.name, k)
            # a range on its own reads seeds left of it as they were given; a by-counter read sets a bit, a logged write names a head entry
            assert all(w[1] < 64 and (r["head_reads"][w[0]] >> w[1]) & 1 for w in r["heads"] if w[1] < 63)
        assert all(live == (1 if (case.subst if lst else case.perfect)[i][3] != mc.RANK_N else 0) for lst, i, live in alone[k]["reads"])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_full_mode_on_the_host_equals_pyref_and_the_replay(case):
    full = run(case, where=ribbit_amd.MERGE_ON_HOST, full=True)
    p, s, a, guards = mc.ref_full(case)
    lists = full["lists"]
    assert (seeds(lists["perfect"]), seeds(lists["subst"]), seeds(lists["anchored"]), lists["guard_hits"]) == (p, s, a, guards)
    assert full["device_merge"][:3] == (0, 0, 0) and full["device_merge"][3] == len(full["cuts"])


def test_a_stride_larger_than_the_words_used_changes_nothing():
    case = [c for c in CASES if c.name == "plane reads"][0]
    xa, stride = packed(case)
    wide = np.zeros((xa.shape[0], stride + 37), dtype="<u4")
    wide[:, :stride] = xa
    wide[:, stride:] = 0xFFFFFFFF
    args = (case.m_lo, case.m_hi, case.length, case.perfect, case.subst, case.calls)
    a = ribbit_amd.debug_merge_ranges(None, *args, xa, stride, where=ribbit_amd.MERGE_ON_HOST, full=True)["lists"]
    b = ribbit_amd.debug_merge_ranges(None, *args, wide, stride + 37, where=ribbit_amd.MERGE_ON_HOST, full=True)["lists"]
    assert seeds(a["anchored"]) == seeds(b["anchored"]) == mc.ref_full(case)[2]


def test_the_mirrors_of_the_structs_have_the_headers_layout(tmp_path):
    """sizeof and every offsetof of RibbitDebugMergeKnobs / RibbitDebugMergeRanges, from the header by the C compiler, against ctypes"""
    import ctypes as C
    import os
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    structs = {"RibbitDebugMergeKnobs": ribbit_amd.DebugMergeKnobs, "RibbitDebugMergeRanges": ribbit_amd.DebugMergeRanges}
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ribbit_hip.h"', "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in mirror._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call([cc, "-I", include, "-o", str(tmp_path / "layout"), str(src)])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    want = {}
    for cname, mirror in structs.items():
        want[cname] = str(C.sizeof(mirror))
        want.update({f"{cname}.{f}": str(getattr(mirror, f).offset) for f, _ in mirror._fields_})
    assert got == want


def test_bad_input_is_refused():
    case = CASES[0]
    xa, stride = packed(case)
    args = (case.m_lo, case.m_hi, case.length, case.perfect, case.subst)
    with pytest.raises(ribbit_amd.RibbitHipError, match="lies outside"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls + [(5, 4, 100, case.length + 1)], xa, stride, where=ribbit_amd.MERGE_ON_HOST)
    with pytest.raises(ribbit_amd.RibbitHipError, match="lies outside"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls + [(5, case.m_hi + 1, 100, 200)], xa, stride, where=ribbit_amd.MERGE_ON_HOST)
    with pytest.raises(ribbit_amd.RibbitHipError, match="open handle"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls, xa, stride, where=ribbit_amd.MERGE_ON_LANES)
    with pytest.raises(ribbit_amd.RibbitHipError, match="only_range"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls, xa, stride, where=ribbit_amd.MERGE_ON_HOST, only_range=10 ** 6)
    # a seed typed for the other list is never retired by the reference's rules: its call would start again without end
    for lists, what in (((case.perfect + [(5, 9, 4, mc.RANK_S)], case.subst), "perfect seed"), ((case.perfect, case.subst + [(5, 9, 4, mc.RANK_P)]), "substitution seed")):
        with pytest.raises(ribbit_amd.RibbitHipError, match=what):
            ribbit_amd.debug_merge_ranges(None, case.m_lo, case.m_hi, case.length, *lists, case.calls, xa, stride, where=ribbit_amd.MERGE_ON_HOST)
    with pytest.raises(ribbit_amd.RibbitHipError, match="knob"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls, xa, stride, where=ribbit_amd.MERGE_ON_HOST, calls_per_range=0)
    with pytest.raises(ribbit_amd.RibbitHipError, match="too short"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls, xa[:, :case.length // 32], case.length // 32, where=ribbit_amd.MERGE_ON_HOST)
    with pytest.raises(ribbit_amd.RibbitHipError, match="two ranges"):
        ribbit_amd.debug_merge_ranges(None, *args, case.calls[:1], xa, stride, where=ribbit_amd.MERGE_ON_HOST)
