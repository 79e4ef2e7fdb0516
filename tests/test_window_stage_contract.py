"""The window stage's contract of tests/window_stage_contract.py, pinned without a GPU: on every constructed record the sequential
call log equals the streak rule (pystreaks.calls_from_streaks) on the same streaks, bounds_hold accepts the bounds of
pystreaks.compact_bounds under every own range and table and rejects bounds that are missing, too low or too high, and every
record still has what its place in the case list promises, so that no case can silently stop reaching its branch.
tests/test_window_stage_gpu.py holds the kernels to the same cases."""
import numpy as np
import pytest

import pystreaks
import window_stage_contract as K

NAMES = [c["name"] for c in K.cases()]
EDGE_DENSE = ["edge_dense", "n_joined", "dense_40k", "large_70k"]


@pytest.mark.parametrize("name", NAMES)
def test_the_sequential_log_equals_the_streak_rule(name):
    c = K.case(name)
    inloop, flush, edge = pystreaks.calls_from_streaks(c["streaks"], c["nmask"])
    assert inloop + flush == K.sequential_log(c)
    assert (inloop, edge) == K.in_loop(c)
    st = c["streaks"]
    assert all(0 <= s < e <= c["L"] and c["m_lo"] <= m <= c["m_hi"] and t in (0, 1, 2) for m, s, e, t in st)
    assert all(a[0] < b[0] or (a[0] == b[0] and a[2] <= b[1]) for a, b in zip(st, st[1:])), "motif-major by start, not overlapping"


@pytest.mark.parametrize("name", NAMES)
def test_bounds_hold_accepts_the_compact_bounds(name):
    c = K.case(name)
    tb = K.tables(c["m_lo"], c["m_hi"])
    for v in K.variants(c):
        kw = {k: x for k, x in v.items() if k != "table"}
        want = K.expectation(c, tb[v["table"]], **kw)
        assert K.bounds_hold(want["calls"], want["pend"], want["seen"]), v
        assert (want["pend"] is None) == (v["full"] or len(want["calls"]) == 0 or want["n_edge"] == 0)
        assert np.all(want["calls"][:, 0] < c["L"] + v["pos_offset"]) and np.all(want["flush"][:, 0] == c["L"] + v["pos_offset"])
        if v["pos_offset"]:
            assert int(want["calls"].max(initial=0)) <= K.INT32_MAX and int(want["flush"].max(initial=0)) <= K.INT32_MAX
    for t in ("subst", "anchored", "nothing"):
        want = K.expectation(c, tb[t])
        for groups, own_lo, own_hi in K.drop_variants(c, t):
            left, ends = K.without(c, groups)
            assert len(left) < len(c["streaks"]) and ends == sorted(set(ends)) and all(0 <= e < c["L"] for e in ends)
            # the groups that stay make the calls they made before: nothing joins across the hole
            inloop, flush, _ = pystreaks.calls_from_streaks(left, c["nmask"])
            gone = {(g[2] + 15, c["streaks"][g[0]][0], c["streaks"][g[0]][1], g[2] + 7) for g in groups}
            assert set(inloop + flush) == set(K.sequential_log(c)) - gone and len(gone) == len(groups)
            assert not gone & {tuple(r) for r in want["calls"].tolist()}, "a dropped call is never a kept one"


def _matters(want):
    """indices of the kept calls whose own bound is needed: an earlier call that was not kept ends beyond them and beyond
    everything the kept calls and their bounds have shown so far"""
    out, running = [], -1
    for i, (end, p, s) in enumerate(zip(want["calls"][:, 3].tolist(), want["pend"].tolist(), want["seen"].tolist())):
        if s > max(end, running):
            out.append(i)
        running = max(running, p, end)
    return out


@pytest.mark.parametrize("name", EDGE_DENSE)
@pytest.mark.parametrize("table", ["second"])
def test_bounds_hold_rejects_bounds_that_are_missing_low_or_high(name, table):
    c = K.case(name)
    want = K.expectation(c, K.tables(c["m_lo"], c["m_hi"])[table])
    calls, pend, seen = want["calls"], want["pend"], want["seen"]
    assert K.bounds_hold(calls, pend, seen)
    assert not K.bounds_hold(calls, None, seen) and not K.bounds_hold(calls, np.full(len(calls), -1), seen)
    matters = _matters(want)
    assert len(matters) >= 3, "edge calls whose bound decides where the cursors stand"
    for i in matters[:25]:
        assert pend[i] == seen[i]
        low, high = pend.copy(), pend.copy()
        low[i] -= 1
        high[i] = seen[i] + 1
        assert not K.bounds_hold(calls, low, seen) and not K.bounds_hold(calls, high, seen), i
    assert not K.bounds_hold(calls[:-1], pend, seen)


# ---- what the case list promises ----------------------------------------------------------------------------------------------

def _terms(c):
    return [t for _, _, _, t in c["streaks"]]


def test_small_and_key_lengths():
    assert [K.case(f"len{n}")["L"] for n in K.SMALL_LENGTHS] == K.SMALL_LENGTHS
    assert all(not K.case(f"len{n}")["streaks"] for n in range(8)) and any(K.case(f"len{n}")["streaks"] for n in (8, 9))
    assert any(len(K.in_loop(K.case(f"len{n}"))[0]) for n in (31, 63, 64, 65))
    assert sum(K.in_loop(K.case("len65_n"))[1]) >= 1
    for n in K.KEY_LENGTHS:
        c = K.case(f"key{n}")
        bits = lambda x: int(x).bit_length()
        assert c["L"] == n and (n in (1016, 2040)) == (bits(n + 8) > bits(n + 7))
        calls, _ = K.in_loop(c)
        assert calls[-1][0] == n - 1 and calls[-1][1] == 2, "a call at the last position of the record"
        assert K.sequential_log(c)[-1][:2] == (n, 3) and K.EOS in _terms(c), "an open streak at the end"
    assert {n + 8 for n in K.KEY_LENGTHS} >= {1023, 1024, 1025, 2047, 2048, 2049}


def test_n_placement():
    c = K.case("n_bits")
    assert {int(p) % 32 for p in np.flatnonzero(c["nmask"])} >= {0, 7, 8, 24, 31} and sum(K.in_loop(c)[1]) >= 5
    c = K.case("n_words")
    e = pystreaks.eval_mask(c["nmask"])[:c["L"] // 32 * 32].reshape(-1, 32)
    empty = np.flatnonzero(~e.any(axis=1))
    calls, edge = K.in_loop(c)
    jumped = [x for x, ed in zip(calls, edge) if ed and (x[3] + 1) // 32 + 1 in empty and not e[(x[3] + 1) // 32, (x[3] + 1) % 32:].any()]
    assert len(empty) >= 10 and jumped, "a call whose first evaluated window lies words behind its end"
    c = K.case("n_block_9000")
    assert c["nmask"][700:9_900].all() and 9_900 - 700 > 8192 and sum(K.in_loop(c)[1]) >= 1
    c = K.case("n_to_the_end")
    assert c["nmask"][-1] and sum(1 for x in K.sequential_log(c) if x[0] == c["L"] and x[3] < c["L"]) >= 2, "unreported groups in the flush"


def test_gaps_and_joins():
    c = K.case("gaps_7_8")
    st = c["streaks"]
    gaps = {(a[3], b[1] - a[2]) for a, b in zip(st, st[1:]) if a[0] == b[0]}
    assert {(K.ZERO, 7), (K.ZERO, 8), (K.N, 8)} <= gaps and not any(t == K.N and g < 8 for t, g in gaps)
    c = K.case("n_joined")
    st = c["streaks"]
    joined = [(a, b) for a, b in zip(st, st[1:]) if a[0] == b[0] and a[3] == K.ZERO and a[2] + 7 >= b[1] and b[3] == K.N]
    assert sum(a[2] + 7 < b[2] for a, b in joined) >= 3, "the group ends before the N-closed streak's last window: reported at the N"
    assert sum(a[2] + 7 >= b[2] for a, b in joined) >= 3, "the group ends behind it: reported at the next evaluated window"


def test_dense_records():
    assert len(K.case("dense_40k")["streaks"]) > 4096 and len(K.case("large_70k")["streaks"]) > 4096
    assert K.groups_of(K.case("periodic")) == [(0, K.PERIODIC_STREAKS), (K.PERIODIC_STREAKS, 2 * K.PERIODIC_STREAKS)] and K.PERIODIC_STREAKS > 2049
    assert K.groups_of(K.case("periodic_cut_2047"))[0] == (0, 2048)
    c = K.case("look_back")
    calls, edge = K.in_loop(c)
    assert calls[0] == (16, 2, 0, 8) and edge == [False, True] and calls[1][0] - calls[0][0] > 8192 + 32
    assert K.expectation(c, [0, 0])["pend"].tolist() == [-1, 8]
    c = K.case("edge_dense")
    calls, edge = K.in_loop(c)
    at = [x[0] for x, e in zip(calls, edge) if e]
    assert len(at) >= 100 and len(at) - len(set(at)) >= 20, "several motifs make edge calls at one position"
    assert c["L"] <= 70_000 and K.case("large_70k")["L"] == 70_000 == max(x["L"] for x in K.cases())


def test_droppable_groups():
    c = K.case("droppable")
    for t in ("subst", "anchored"):
        groups = K.droppable(c, K.tables(6, 9)[t])
        assert {16, 17, 31} <= {g[2] % 32 for g in groups}
        mid = [g for g in groups if (g[2] + 15) % 32 not in (0, 31)]
        assert len(mid) >= 3 and len(K.drop_variants(c, t)) >= 4 + 6 * 3 + 2
    c = K.case("drop_tail")
    last = max(K.droppable(c, K.tables(6, 9)["subst"]), key=lambda g: g[2])
    calls, _ = K.in_loop(c)
    assert calls[-1] == (last[2] + 15, 6, c["streaks"][last[0]][1], last[2] + 7) and calls[-1][3] == max(x[3] for x in calls)
    assert not [x for x in K.sequential_log(c) if x[0] == c["L"]]
