"""GPU tests of the window-stage kernels (ribbit_amd/csrc/window_stage.hip) and their orchestration on constructed pass-streaks:
every case of tests/window_stage_contract.py goes through ribbit_hip_debug_window_calls, in both stage slots, compact and full, and
must return exactly what the contract cuts out of the sequential call log -- kept calls, end-of-sequence calls, tail_pend, inexact,
the number of edge calls, the cursor bounds one by one, and bounds that move a merge's cursors as the full list would.  Groups the
anchored scan's filter may drop are handed over once as streaks and once as dropped ends; the edge-call list is made to overflow;
a large batch is followed by small ones on one handle; malformed streak lists are refused before a kernel runs.  All compared
values are integers: equality throughout."""
import numpy as np
import pytest

import ribbit_amd
import window_stage_contract as K
from ribbit_amd import RUN_DT, STAGE_ANCHORED, STAGE_SUBST

pytestmark = pytest.mark.gpu
SLOTS = (STAGE_SUBST, STAGE_ANCHORED)
NAMES = [c["name"] for c in K.cases()]
DROP_CASES = ["droppable", "drop_tail", "len65", "key2040", "n_joined", "dense_40k", "large_70k"]


@pytest.fixture(scope="module")
def scanner():
    made = {}

    def get(m_lo, m_hi):
        if (m_lo, m_hi) not in made:
            made[(m_lo, m_hi)] = ribbit_amd.Scanner(m_lo, m_hi)
        return made[(m_lo, m_hi)]
    yield get
    for sc in made.values():
        sc.close()


def _records(c):
    if "records" not in c:
        c["records"] = K.records_of(c["streaks"])
    return c["records"]


def _call(sc, c, v, slot, records=None, **more):
    table = K.tables(c["m_lo"], c["m_hi"])[v["table"]]
    kw = {k: x for k, x in v.items() if k != "table"}
    return sc.debug_window_calls(slot, _records(c) if records is None else records, min_span=None if v["full"] else table, **kw, **more)


def _want(c, v):
    return K.expectation(c, K.tables(c["m_lo"], c["m_hi"])[v["table"]], **{k: x for k, x in v.items() if k != "table"})


def _check(got, want, where):
    rows = lambda a: a.view("<i4").reshape(-1, 4)
    assert np.array_equal(rows(got["calls"]), want["calls"]), f"{where}: calls"
    assert np.array_equal(rows(got["flush"]), want["flush"]), f"{where}: end-of-sequence calls"
    assert got["tail_pend"] == want["tail_pend"], f"{where}: tail_pend"
    assert got["inexact"] == want["inexact"], f"{where}: inexact"
    assert got["n_edge"] == want["n_edge"], f"{where}: edge calls counted"
    assert (got["pend"] is None) == (want["pend"] is None), f"{where}: pend present"
    assert K.bounds_hold(got["calls"], got["pend"], want["seen"]), f"{where}: the bounds move the cursors as the full list does"
    assert want["pend"] is None or np.array_equal(got["pend"], want["pend"]), f"{where}: pend"


@pytest.mark.parametrize("name", NAMES)
def test_constructed_streaks_give_the_calls_of_the_sequential_log(scanner, name):
    c = K.case(name)
    sc = scanner(c["m_lo"], c["m_hi"])
    sc.load_record(c["seq"])
    for v in K.variants(c):
        want = _want(c, v)
        for slot in SLOTS:
            _check(_call(sc, c, v, slot), want, f"{name} {v} slot {slot}")


@pytest.mark.parametrize("name", DROP_CASES)
def test_dropped_groups_leave_what_their_calls_would_have_left(scanner, name):
    c = K.case(name)
    sc = scanner(c["m_lo"], c["m_hi"])
    sc.load_record(c["seq"])
    ran = 0
    for t in ("subst", "anchored", "nothing"):
        for groups, own_lo, own_hi in K.drop_variants(c, t):
            v = dict(table=t, full=False, own_lo=own_lo, own_hi=own_hi, z_lo=0, keep_flush=True, pos_offset=0)
            want = _want(c, v)
            left, ends = K.without(c, groups)
            where = f"{name} table {t} own [{own_lo}, {own_hi}) dropped ends {ends[:8]}"
            _check(_call(sc, c, v, SLOTS[ran % 2]), want, where + " (present)")
            _check(_call(sc, c, v, SLOTS[ran % 2], records=K.records_of(left), dropped_ends=ends), want, where + " (dropped)")
            ran += 1
    assert ran >= 3


def test_an_edge_list_that_overflows_is_sized_again():
    c = K.case("edge_dense")
    v = dict(table="second", full=False, own_lo=0, own_hi=K.OWN_ALL, z_lo=0, keep_flush=True, pos_offset=0)
    want = _want(c, v)
    assert want["n_edge"] >= 100
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:          # a fresh handle: its edge list has no room yet
        sc.load_record(c["seq"])
        for cap in (1, 4, want["n_edge"] - 1, want["n_edge"], 0, 1):
            for slot in SLOTS:
                got = _call(sc, c, v, slot, first_edge_cap=cap)
                _check(got, want, f"edge capacity {cap} slot {slot}")
                assert cap in (0, want["n_edge"]) or got["n_edge"] > cap, "the first list was too small: the retry ran"


def test_a_smaller_batch_after_a_larger_one_sees_nothing_of_it():
    big, small = K.case("dense_40k"), [K.case(n) for n in ("n_bits", "n_to_the_end", "edge_dense", "drop_tail")]
    assert all((x["m_lo"], x["m_hi"]) == (big["m_lo"], big["m_hi"]) and x["L"] < big["L"] // 4 for x in small)
    v = dict(table="second", full=False, own_lo=0, own_hi=K.OWN_ALL, z_lo=0, keep_flush=True, pos_offset=0)
    with ribbit_amd.Scanner(big["m_lo"], big["m_hi"]) as sc:
        for c in [big] + small + [big, small[0]]:
            sc.load_record(c["seq"])
            for vv in (v, dict(v, table="subst"), dict(v, table="zero", full=True)):
                _check(_call(sc, c, vv, STAGE_ANCHORED), _want(c, vv), f"{c['name']} after the others, {vv}")
            groups = K.droppable(c, K.tables(c["m_lo"], c["m_hi"])["subst"])[:40]
            if groups:
                left, ends = K.without(c, groups)
                vv = dict(v, table="subst")
                _check(_call(sc, c, vv, STAGE_ANCHORED, records=K.records_of(left), dropped_ends=ends), _want(c, vv), f"{c['name']} with dropped groups")


def _streaks(*rows):
    return K.records_of([tuple(r) for r in rows])


def test_two_open_streaks_of_one_motif_raise_the_stage_flag(scanner):
    sc = scanner(2, 3)
    sc.load_record(b"A" * 200)
    with pytest.raises(ribbit_amd.RibbitHipError, match=r"flags 0x1\)"):
        sc.debug_window_calls(STAGE_SUBST, _streaks((2, 10, 40, K.EOS), (2, 100, 193, K.EOS)), min_span=[0, 0])
    # the handle is as good as before
    c = K.case("gaps_7_8")
    sc.load_record(c["seq"])
    v = K.variants(c)[0]
    _check(_call(sc, c, v, STAGE_SUBST), _want(c, v), "after the flagged call")


def test_malformed_input_is_refused_on_the_host(scanner):
    sc = scanner(2, 3)
    sc.load_record(b"A" * 100 + b"N" + b"A" * 99)
    ok = [(2, 10, 40, K.ZERO), (2, 60, 80, K.ZERO), (3, 5, 30, K.ZERO)]
    sc.debug_window_calls(STAGE_SUBST, _streaks(*ok), min_span=[0, 0])
    bad = {"order": [ok[1], ok[0], ok[2]], "order ": [ok[2], ok[0], ok[1]], "order  ": [ok[0], ok[0], ok[2]],
           "overlaps": [ok[0], (2, 39, 80, K.ZERO), ok[2]],
           "no stretch": [ok[0], (2, 60, 201, K.ZERO), ok[2]], "no stretch ": [(2, -1, 40, K.ZERO)], "no stretch  ": [(2, 40, 40, K.ZERO)],
           "motif": [ok[0], (4, 60, 80, K.ZERO)], "motif ": [(1, 10, 40, K.ZERO), ok[0]], "term": [(2, 10, 40, 3)], "term ": [(2, 10, 40, -1)]}
    for why, rows in bad.items():
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: streak [0-9]+: .*{why.strip()}"):
            sc.debug_window_calls(STAGE_SUBST, _streaks(*rows), min_span=[0, 0])
    for kw, why in ((dict(dropped_ends=[200]), "outside the record"), (dict(dropped_ends=[-1]), "outside the record"),
                    (dict(dropped_ends=[50, 50]), "not ascending"), (dict(own_lo=5, own_hi=4), "geometry"), (dict(own_lo=-1), "geometry"),
                    (dict(pos_offset=K.INT32_MAX - 199), "geometry"), (dict(pos_offset=-1), "geometry"), (dict(z_lo=-1), "geometry"),
                    (dict(first_edge_cap=2**24 + 1), "bad size")):
        with pytest.raises(ribbit_amd.RibbitHipError, match=f"error -1: .*{why}"):
            sc.debug_window_calls(STAGE_SUBST, _streaks(*ok), min_span=[0, 0], **kw)
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: stage"):
        sc.debug_window_calls(0, _streaks(*ok), min_span=[0, 0])
    with pytest.raises(ribbit_amd.RibbitHipError, match="error -1: null"):
        sc.debug_window_calls(STAGE_SUBST, _streaks(*ok))                     # compact form without a table
    with ribbit_amd.Scanner(2, 3) as fresh, pytest.raises(ribbit_amd.RibbitHipError, match="error -3: no record loaded"):
        fresh.debug_window_calls(STAGE_SUBST, np.zeros(0, RUN_DT), min_span=[0, 0])
    # the largest offset there is, and the streaks as they are, go through
    got = sc.debug_window_calls(STAGE_SUBST, _streaks(*ok), min_span=[0, 0], pos_offset=K.INT32_MAX - 200)
    assert len(got["calls"]) == 3 and int(got["calls"]["pos"].min()) > K.INT32_MAX - 200
