"""The seed-scan kernels (seed_longest_run_kernel, sym_kernel, long_motif_rows_kernel, small_motifs_kernel) on constructed seed
lists: a handle loads a record, adopts a list of tests/seed_scan_contract.py through ribbit_hip_adopt_dispatch, and what the
device computes is compared with the plain statement of the reference there, with the oracle (which adopts the same list) and
with the host twin.  tests/test_seed_scans.py proves on the CPU that the lists hold the edges they are made for."""
import numpy as np
import pytest

import ribbit_amd
import seed_scan_contract as K

pytestmark = pytest.mark.gpu

BY_NAME = K.cases_by_name()


def _adopted(sc, c):
    sc.load_record(c["seq"])
    sc.adopt_dispatch(c["seeds"])
    assert np.array_equal(sc.dispatch_seeds().view("<i4"), c["seeds"].view("<i4"))


# ---------------------------------------------------------------------------------------------------------------- longest runs
@pytest.mark.parametrize("name", list(BY_NAME))
def test_longest_runs_and_jobs_of_a_constructed_list(name):
    """seed_longest_run_kernel against parse_seed.cpp:26-44 on the oracle's planes and against the host twin; then the jobs and
    motif strings (small_motifs_kernel for m <= 10; sym_kernel and long_motif_rows_kernel beyond: the row chosen among ties, row 0
    of the record without a score, seeds at both ends of the record) against the oracle's"""
    c = BY_NAME[name]
    _, wjobs, longest, _ = K.oracle_of(name)
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        got = sc.seed_longest_runs()
        bad = np.nonzero(got != longest)[0]
        assert len(bad) == 0, (name, c["seeds"][bad[:5]], got[bad[:5]], longest[bad[:5]])
        assert np.array_equal(got, ribbit_amd.host_longest_runs(c["m_lo"], c["m_hi"], c["seq"], c["seeds"]))
        K.assert_same_jobs(sc.refine_jobs(K.library_params(c)), wjobs, name)


# ------------------------------------------------------------------------------------------------------------ long-motif rows
LONG = [n for n in BY_NAME if n.startswith(("rows_m", "last_row", "positions_m", "mixed_"))] + ["selection"]


@pytest.mark.parametrize("name", LONG)
def test_best_rows_are_mostFrequentLongerMotifs(name):
    """the row long_motif_rows_kernel hands back for every seed against parse_seed.cpp:153-256 as best_row states it: the first of
    tied rows, row 0 of the record without a score, the last row where only that one wins, every slice count, seeds at both ends of
    the record; -1 for the seeds that are not asked"""
    c = BY_NAME[name]
    want, _ = K.best_rows_of(name)
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        got = sc.seed_best_rows(K.library_params(c))
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (name, c["seeds"][bad[:5]], got[bad[:5]], want[bad[:5]])
        assert name == "selection" or (want >= 0).sum() >= 4


# ------------------------------------------------------------------------------------------------------- the small-motif table
def _table(sc, c):
    head, rec = sc.small_motifs(K.library_params(c))
    return head, rec, K.assert_table_matches(c, head, rec, sc.seed_longest_runs())


@pytest.mark.parametrize("name", [c["name"] for c in K.small_table_cases()])
def test_small_motif_table_is_possibleMotifs(name):
    """head and records of small_motifs_kernel against expected_head_and_records: seed lengths around the warm-up and the 64-position
    loads, the first N everywhere it can cut, the record's end, the 3m gap, 64 / 65 classes, 64 / 65 early reports, the record layout"""
    c = BY_NAME[name]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        head, rec, flags = _table(sc, c)
        if name == "limits":
            for kind, m, v, i in c["checks"]:
                if kind == "classes":
                    assert int(flags[i]) == (0 if v == 64 else 1), (m, v, head[i])
                    assert v != 64 or int(head[i, 2]) == 64          # every class left the device
                else:
                    assert int(flags[i]) == 0
            gaps = {(m, v): int(head[i, 1]) for kind, m, v, i in c["checks"] if kind == "gap"}
            for m in range(1, 11):
                assert gaps[(m, 3 * m + 1)] == gaps[(m, 3 * m)] + 1, (m, gaps)
        elif "n_early" in c:
            assert int(flags[0]) == (0 if c["n_early"] == 64 else 1)
            assert c["n_early"] != 64 or (int(head[0, 1]), int(head[0, 2])) == (64, 1)
        elif name == "layout":
            assert [int(x) for x in flags] == [0, 0, 0, 0]
            assert [int(x) for x in head[:2, 2]] == [0, 1] and int(head[2, 2]) >= 2 and int(head[3, 2]) >= 5
        else:
            assert (flags == 0).all()


def test_selection_by_longest_run_and_motif_length():
    """default threshold 3: a longest run of 2 has no device result, one of 3 has, m = 11 has none"""
    c = BY_NAME["selection"]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        assert [int(x) for x in sc.seed_longest_runs()] == c["longest"]
        _, _, flags = _table(sc, c)
        assert [int(x) for x in flags] == c["flags"]


def test_record_arena_full():
    """flags 2: with room for half of the records, a seed has its records or is left to the host twin; the jobs are the oracle's
    either way, refinement counts both kinds, and the automatic capacity serves every seed again"""
    c = BY_NAME["arena"]
    _, wjobs, _, _ = K.oracle_of("arena")
    n, per = len(c["seeds"]), c["records_per_seed"]
    cap = n * per // 2
    rp = K.library_params(c)
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        sc.debug_set_small_record_capacity(cap)
        head, rec = sc.small_motifs(rp)
        assert set(int(x) for x in head[:, 3]) == {0, 2}
        served = head[:, 3] == 0
        assert int(served.sum()) == cap // per                   # every seed asks for `per` records: the first cap // per fit
        assert len(rec) <= cap and int(head[served, 0].max()) + per <= cap
        p = K.params_of(c)                                       # every seed of the list is the same seed: one expectation
        want = K.expected_head_and_records(c["seq"], int(c["seeds"][0]["start"]), int(c["seeds"][0]["end"]), 3, p["min_length"][3],
                                           p["perfect_units"][3], 0, 0)
        assert want[0] == 0 and len(want[3]) == per
        irec = rec.astype(np.int64)
        for i in np.nonzero(served)[0]:
            assert (int(head[i, 1]), int(head[i, 2])) == (want[1], want[2])
            assert np.array_equal(irec[int(head[i, 0]):int(head[i, 0]) + per], want[3]), i
        K.assert_same_jobs(sc.refine_jobs(rp), wjobs, "arena")
        before = ribbit_amd.small_motif_counters()
        sc.refine_bed("arena", rp)
        after = ribbit_amd.small_motif_counters()
        assert (after[0] - before[0], after[1] - before[1]) == (cap // per, n - cap // per)
        sc.debug_set_small_record_capacity(0)
        head, rec = sc.small_motifs(rp)
        assert (head[:, 3] == 0).all() and len(rec) == n * per
        K.assert_table_matches(c, head, rec, sc.seed_longest_runs())


# ------------------------------------------------------------------------------------------------------ end to end, rejection
@pytest.mark.parametrize("name", [c["name"] for c in K.mixed_cases()])
def test_bed_of_a_mixed_constructed_list(name):
    c = BY_NAME[name]
    o = K.oracle_of(name)[0]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        _adopted(sc, c)
        text = sc.refine_bed("mixed")
        assert text == o.refine_bed("mixed") and text.count("\n") >= 10


def test_adopt_dispatch_rejects_seeds_the_kernels_cannot_index():
    """RIBBIT_E_ARG naming the first offending index, before anything on the handle changes: nothing is launched for such a list,
    and the list the handle had still refines to the same text"""
    c = BY_NAME["mixed_2_40"]
    L = len(c["seq"])
    with ribbit_amd.Scanner(2, 40) as sc:
        _adopted(sc, c)
        text = sc.refine_bed("r")
        for k, (bad, why) in enumerate(K.rejected_seeds(L, 2, 40)):
            at = (0, 7, len(c["seeds"]))[k % 3]
            lst = np.concatenate([c["seeds"][:at], K.seeds_of([bad, bad]), c["seeds"][at:]])
            with pytest.raises(ribbit_amd.RibbitHipError, match=rf"error -1: seed {at} of the adopted list"):
                sc.adopt_dispatch(lst)
            assert np.array_equal(sc.dispatch_seeds().view("<i4"), c["seeds"].view("<i4")), why
        assert sc.refine_bed("r") == text
        sc.adopt_dispatch(K.seeds_of([(0, 0, 2), (L, L, 40), (0, L, 40)]))      # the bounds themselves are inside
        assert len(sc.seed_longest_runs()) == 3
    with ribbit_amd.Scanner(2, 12) as sc:                                         # a motif longer than the record
        sc.load_record(b"ACGTACGTAC")
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: seed 0 of the adopted list"):
            sc.adopt_dispatch(K.seeds_of([(0, 10, 11)]))
        sc.adopt_dispatch(K.seeds_of([(0, 10, 10)]))
