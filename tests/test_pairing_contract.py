"""The pairing contract of tests/pairing_contract.py, pinned without a GPU: its plain pairing equals the library's host pairing
(ribbit_host_perfect_runs_from_events) on every constructed stream and on the events of two oracle records, its own-range rule equals
the chunk contract (chunk_contract._chunk_runs) at every cut, and its layouts read back as the streams they were made from.
tests/test_pairing_sharded_gpu.py holds the pairing kernels to the same cases."""
import numpy as np
import pytest

import pairing_contract as K
import pyevents
import ribbit_amd
from cases import edge_cases, simulated_cases
from chunk_contract import _chunk_runs, oracle_runs
from oracle_lib import Oracle

BY_NAME = K.cases_by_name()
WELL_FORMED = [c["name"] for c in K.well_formed_cases()]


def _host_pairing(stream, m_lo, m_hi):
    words = np.array([K.pack(*e) for e in stream], dtype="<u8")
    counts = np.bincount([e[1] - m_lo for e in stream], minlength=m_hi - m_lo + 1).astype("<u8")
    return ribbit_amd.host_perfect_runs_from_events(m_lo, m_hi, [words], [counts])


def _rows(records):
    return [tuple(int(x) for x in r) for r in records]


def test_the_generators_build_what_they_promise():
    """the generators assert their own shapes (a full region, single-event chunks, the 601-event chunk, the region sizes of the grid
    stride, the block counts) while they build; building them all is the check"""
    assert len(BY_NAME) >= 35
    assert all(BY_NAME[c["name"]] is c for c in K.well_formed_cases())
    assert {c["nm"] * c["ntile"] for c in K.prefix_cases()} == {1023, 1024, 1025, 2049, 4 * 1024 + 3}
    assert [(c["nm"] * c["ntile"] + 1023) // 1024 for c in K.carry_cases()] == [255, 256, 257, 513]
    assert [int(c["counters"].max()) for c in K.grid_stride_cases()] == [16384, 16385, 40001]


@pytest.mark.parametrize("name", WELL_FORMED)
def test_pair_equals_the_host_pairing(name):
    c = BY_NAME[name]
    slots, halves = K.pair(c["stream"], c["m_lo"], c["nm"], c["length"], *K.WHOLE)
    assert halves == [] and len(slots) * 2 == len(c["stream"])
    assert slots == _rows(_host_pairing(c["stream"], c["m_lo"], c["m_hi"]))


@pytest.mark.parametrize("name", WELL_FORMED + ["two_halves_per_motif"])
def test_layout_reads_back_as_its_stream(name):
    """regions in order, each cut at its cap, then every motif's chunks in tile order: the stream in (motif, position) order"""
    c = BY_NAME[name]
    dense, summary, overflow, table, status = K.dense_and_table(c["events"], c["counters"], c["region_cap"], c["m_lo"], c["nm"], c["length"])
    assert status == 0 and summary == len(c["stream"]) and overflow == (name == "clamp")
    assert K.motif_streams(dense, table, c["m_lo"], c["nm"]) == c["stream"]


def test_malformed_cases_are_refused_by_the_contract_and_marked_in_the_table():
    for c in K.malformed_cases():
        dense, _, _, table, status = K.dense_and_table(c["events"], c["counters"], c["region_cap"], c["m_lo"], c["nm"], c["length"])
        assert status == {"dup_chunk_in_two_shards": 2, "motif_outside_the_launch_in_shard_1": 1}.get(c["name"], 0), c["name"]
        if status == 0:
            with pytest.raises(ValueError):
                K.pair(K.motif_streams(dense, table, c["m_lo"], c["nm"]), c["m_lo"], c["nm"], c["length"], *K.WHOLE)


ORACLE_RECORDS = [c for c in edge_cases() if c[0] == "n_runs"] + [c for c in simulated_cases() if c[0] == "sim_cfg2_120k"]


@pytest.mark.parametrize("name,seq,m_lo,m_hi", ORACLE_RECORDS, ids=[c[0] for c in ORACLE_RECORDS])
def test_pair_on_an_oracle_records_events_equals_its_runs(name, seq, m_lo, m_hi):
    with Oracle(seq, m_lo, m_hi) as o:
        words, _ = pyevents.perfect_events(o, m_lo, m_hi)
        want = oracle_runs(o, m_lo, m_hi)
    slots, halves = K.pair([K.unpack(w) for w in words], m_lo, m_hi - m_lo + 1, len(seq), *K.WHOLE)
    assert len(want) > 0 and halves == [] and slots == _rows(want)


def test_own_range_rule_equals_the_chunk_contract_at_every_cut():
    truth = K.shard_truth()
    stream = K.events_of(truth)
    runs = K.as_records(truth)
    ranges = K.own_ranges(truth, K.SHARD_LENGTH)
    assert len(ranges) > 500
    seen = {"whole": 0, "start": 0, "end": 0, "covered": 0}
    for own_lo, own_hi in ranges:
        slots, halves = K.pair(stream, *K.SHARD_M[:1], 19, K.SHARD_LENGTH, own_lo, own_hi, 0)
        whole, cut = _chunk_runs(runs, own_lo, own_hi)
        assert len(slots) == len(truth)
        assert [s for s in slots if s[3] != K.NOT_OWNED] == _rows(whole), (own_lo, own_hi)
        assert sorted(halves) == sorted(_rows(cut)), (own_lo, own_hi)
        seen["whole"] += len(whole)
        seen["start"] += sum(h[3] == K.HALF_START for h in halves)
        seen["end"] += sum(h[3] >= K.HALF_END for h in halves)
        seen["covered"] += sum(r[0] < own_lo and r[1] >= own_hi for r in truth) if own_hi > own_lo else 0
    assert all(seen.values()), seen


def test_pos_offset_shifts_every_position_and_nothing_else():
    truth = K.shard_truth()
    stream = K.events_of(truth)
    off = 2 ** 31 - 1 - K.SHARD_LENGTH
    base = K.pair(stream, 2, 19, K.SHARD_LENGTH, 30000, 60000, 0)
    moved = K.pair(stream, 2, 19, K.SHARD_LENGTH, 30000, 60000, off)
    shift = lambda r: tuple(x + off if x >= 0 else x for x in r[:2]) + r[2:]          # (-1 marks the missing end of a half)
    assert moved == ([r if r[3] == K.NOT_OWNED else shift(r) for r in base[0]], [shift(r) for r in base[1]])
    assert max(r[1] for r in moved[0] + moved[1]) <= 2 ** 31 - 1
