"""The seed scans on constructed seed lists, CPU side (no GPU): the plain statement of tests/seed_scan_contract.py is pinned to
the oracle (which adopts a list through rbo_set_dispatch), and the host twins (ribbit_host_longest_runs, ribbit_host_refine_jobs
without composed planes) equal the oracle on every list.  tests/test_seed_scans_gpu.py hands the same lists to the device."""
from collections import Counter

import numpy as np
import pytest

import ribbit_amd
import seed_scan_contract as K
from cases import edge_cases, large_motif_cases, simulated_cases
from oracle_lib import Oracle

BY_NAME = K.cases_by_name()
CASES = list(BY_NAME.values())
IDS = list(BY_NAME)


oracle_of = K.oracle_of


def test_every_generator_precondition_holds():
    """the generators assert their own preconditions (64 / 65 classes, K - 1 early reports, the gap boundary, N positions, row
    counts) when they build their cases; building them is the check"""
    assert len(CASES) == len(BY_NAME) >= 25


@pytest.mark.parametrize("name", [c["name"] for c in K.longest_run_cases()])
def test_longest_run_cases_hold_the_edges_they_are_made_for(name):
    c = BY_NAME[name]
    _, _, longest, planes = oracle_of(name)
    where = Counter(K.where_longest(planes[int(s["mlen"])], int(s["start"]), int(s["end"])) for s in c["seeds"])
    if name == "all_A_1000":
        assert all(int(l) == int(s["end"]) - int(s["start"]) for l, s in zip(longest, c["seeds"]))      # whole words, every seed
        assert int(longest.max()) >= 96 + 31
    else:
        assert where["first"] > 0 and where["last"] > 0 and where["inside"] > 0 and where["only"] > 0, where
        assert where["none"] > 0 or (longest == 0).any()
    assert (c["seeds"]["start"] == c["seeds"]["end"]).any() and (c["seeds"]["end"] == len(c["seq"])).any()


@pytest.mark.parametrize("name", IDS)
def test_host_twins_equal_the_oracle(name):
    c = BY_NAME[name]
    _, wjobs, longest, _ = oracle_of(name)
    got = ribbit_amd.host_longest_runs(c["m_lo"], c["m_hi"], c["seq"], c["seeds"])
    assert np.array_equal(got, longest)
    gjobs = ribbit_amd.host_refine_jobs(c["m_lo"], c["m_hi"], c["seq"], None, 0, c["seeds"], K.library_params(c))
    K.assert_same_jobs(gjobs, wjobs, name)


SMALL = [c["name"] for c in K.small_table_cases()] + ["selection", "arena"]


@pytest.mark.parametrize("name", SMALL)
def test_small_motif_contract_is_the_oracles(name):
    """per seed: the early reports are the oracle's first small jobs (query_start, query_length) in order, the survivors the
    rest as a multiset (their order is the unordered_map's)"""
    c = BY_NAME[name]
    p = K.params_of(c)
    _, (jobs, _), longest, _ = oracle_of(name)
    seen = 0
    for i, s in enumerate(c["seeds"] if name != "arena" else c["seeds"][:3]):
        m = int(s["mlen"])
        mine = jobs[jobs["seed_index"] == i]
        if m > 10:
            continue
        if longest[i] < p["threshold"]:
            assert len(mine) == 0
            continue
        assert (mine["small"] == 1).all()
        early, classes = K.small_motif_table(c["seq"], int(s["start"]), int(s["end"]), m, p["min_length"].get(m, 0), p["perfect_units"].get(m, 0))
        got = [(int(j["query_start"]), int(j["query_length"])) for j in mine]
        want_early = [(e[1], e[2] - e[1]) for e in early]
        assert got[:len(early)] == want_early, (name, i, s)
        want_rest = [(k["first"], k["last"] - k["first"]) for k in classes if K.qualifies(k, p["min_length"].get(m, 0), p["perfect_units"].get(m, 0))]
        assert Counter(got[len(early):]) == Counter(want_rest), (name, i, s)
        seen += len(got)
    assert seen > 0 or name == "selection"
    if "n_early" in c:
        assert len(jobs) == c["n_early"] + 1                    # K jobs: K - 1 early reports and the survivor


LONG = [c["name"] for c in K.long_row_cases() + [K.last_row_case()] + K.long_position_cases()]


@pytest.mark.parametrize("name", LONG)
def test_best_row_is_the_oracles_motif_and_the_inputs_hold_ties_and_zero_scores(name):
    c = BY_NAME[name]
    _, (jobs, pool), _, _ = oracle_of(name)
    motifs = dict(zip((int(j["seed_index"]) for j in jobs), K.motifs_of(jobs, pool)))
    sym = K.encode(c["seq"])
    kinds = Counter()
    for i, s in enumerate(c["seeds"]):
        start, end, m = int(s["start"]), int(s["end"]), int(s["mlen"])
        ssl = K.seed_sequence_length(sym, start, end, m)
        row, score, ties = K.best_row(c["seq"], start, ssl, m)
        want = c.get("expect", [None] * len(c["seeds"]))[i]
        if want == "last":
            assert row == start + ssl - m and ties == 1 and score > 0, (name, i, row, score, ties)
        if want == "tie":
            assert ties >= 2 and score > 0, (name, i, ties, score)      # several rows of an exact repeat reach the best score: the first wins
        if want == "zero":
            assert score == 0 and row == 0, (name, i, row, score)
        kinds[want] += 1
        atom, motif = K.long_motif(c["seq"], row, m)
        if end - start < 0.9 * m or m % atom != 0:               # parse_seed.cpp:363, :394
            assert i not in motifs
            continue
        assert motifs[i] == motif, (name, i, s, row, score)
        if want == "zero":
            assert motif == K.long_motif(c["seq"], 0, m)[1] and motif != K.long_motif(c["seq"], start, m)[1]
    if name.startswith("rows_m"):
        assert kinds["tie"] >= 1 and kinds["zero"] >= 3, kinds


def test_set_dispatch_rejects_what_the_refinement_half_cannot_index():
    c = BY_NAME["layout"]
    with Oracle(c["seq"], 2, 12) as o:
        o.run_all()
        o.set_dispatch(c["seeds"])
        before = o.refine_jobs()
        L = len(c["seq"])
        for bad, why in K.rejected_seeds(L, 2, 12):
            lst = np.concatenate([c["seeds"], K.seeds_of([bad])])
            with pytest.raises(ValueError):
                o.set_dispatch(lst)
            assert np.array_equal(o.dispatch().view("<i4"), c["seeds"].view("<i4")), why      # the list stays as it was
        K.assert_same_jobs(o.refine_jobs(), before)
        o.set_dispatch(K.seeds_of([(0, 0, 2), (L, L, 12), (0, L, 12)]))                       # the bounds themselves are inside
        o.set_dispatch(np.zeros(0, K.SEED_DT))
        assert len(o.dispatch()) == 0 and len(o.refine_jobs()[0]) == 0
    with Oracle(b"ACGTACGTAC", 2, 12) as o:                                                   # a motif longer than the record
        o.run_all()
        with pytest.raises(ValueError):
            o.set_dispatch(K.seeds_of([(0, 10, 11)]))
        o.set_dispatch(K.seeds_of([(0, 10, 10)]))


NATURAL = edge_cases() + simulated_cases() + large_motif_cases()


@pytest.mark.parametrize("name,seq,m_lo,m_hi", NATURAL, ids=[c[0] for c in NATURAL])
def test_every_natural_dispatch_list_passes_the_rule(name, seq, m_lo, m_hi):
    """what ribbit_hip_adopt_dispatch and rbo_set_dispatch demand of a seed (one rule, include/ribbit_hip.h) holds for every list
    the stages make: adopting a record's own list never fails"""
    with Oracle(seq, m_lo, m_hi) as o:
        o.run_all()
        d = o.dispatch()
        o.set_dispatch(d)
        assert np.array_equal(o.dispatch().view("<i4"), d.view("<i4"))
        assert len(d) == 0 or (d["start"].min() >= 0 and (d["start"] <= d["end"]).all() and d["end"].max() <= len(seq)
                               and d["mlen"].min() >= m_lo and d["mlen"].max() <= min(m_hi, len(seq)))
