"""The pairing kernels (pair_chunk_bounds / _chunk_starts / _scan_partials / _run_base / _runs / _publish) and the legacy pair
(compact_events_kernel, chunk_table_kernel) on constructed event streams dealt over the 64 regions, held to the plain contract of
tests/pairing_contract.py (pinned on the CPU by tests/test_pairing_contract.py).  Every test opens one Scanner and loads nothing:
ribbit_hip_debug_pair_events_sharded places the events and counters as given.  All compared values are integers: equality throughout.

Two places where the cases differ from a literal reading of their list, both forced by what a well-formed stream is:
  * a region cannot hold an odd number of events of one motif and nothing else be anywhere: at 16385 and 40001 events the END of the last
    run, a chunk of its own, lies in region 0 (pairing_contract.grid_stride_cases);
  * the large tables use motifs 2..990, the widest range a handle takes (989 motifs: 255, 256, 257 and 513 blocks of 1024 entries), and
    an END at or below its START can only be met inside a chunk, since chunks are cut by position (pairing_contract.malformed_cases).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pairing_contract as K
import ribbit_amd

pytestmark = pytest.mark.gpu
BY_NAME = K.cases_by_name()


def names(cases):
    return [c["name"] for c in cases]


@functools.lru_cache(maxsize=None)
def legacy(name):
    c = BY_NAME[name]
    return K.dense_and_table(c["events"], c["counters"], c["region_cap"], c["m_lo"], c["nm"], c["length"])


def first_difference(got, want):
    n = min(len(got), len(want))
    differ = np.flatnonzero(got[:n] != want[:n])
    at = int(differ[0]) if len(differ) else n
    return f"{len(got)} records for {len(want)}; first difference at {at}: got {got[at:at + 2]}, want {want[at:at + 2]}"


def pair_on_gpu(sc, c, own=None):
    own_lo, own_hi, pos_offset = own or (c["own_lo"], c["own_hi"], c["pos_offset"])
    return sc.debug_pair_events_sharded(c["events"], c["counters"], c["region_cap"], c["length"], own_lo, own_hi, pos_offset)


def check_pairing(c, got, own=None):
    """slots in order, halves in any order, the three status words, the published counters"""
    own_lo, own_hi, pos_offset = own or (c["own_lo"], c["own_hi"], c["pos_offset"])
    slots, halves = K.pair(c["stream"], c["m_lo"], c["nm"], c["length"], own_lo, own_hi, pos_offset)
    tag = (c["name"], own_lo, own_hi, pos_offset)
    assert got["flags"] == 0, tag
    assert got["total"] == len(slots), tag
    want = K.as_records(slots)
    assert np.array_equal(got["runs"], want), (tag, first_difference(got["runs"], want))
    assert got["n_halves"] == len(halves), tag
    assert sorted(tuple(int(x) for x in h) for h in got["halves"]) == sorted(halves), tag
    assert np.array_equal(got["published"], c["counters"]), tag
    return slots, halves


def check_legacy(c, got):
    """the dense stream, EV_SUMMARY, the overflow word, the (motif, tile) table and its status"""
    dense, summary, overflow, table, status = legacy(c["name"])
    assert (got["summary"], got["overflow"], got["table_status"]) == (summary, overflow, status), c["name"]
    assert np.array_equal(got["dense"], dense), (c["name"], first_difference(got["dense"], dense))
    if not np.array_equal(got["table"], table):
        mi, tile = (int(x[0]) for x in np.nonzero((got["table"] != table).any(axis=2)))
        raise AssertionError(f"{c['name']}: table entry (motif {c['m_lo'] + mi}, tile {tile}): got {got['table'][mi, tile]}, want {table[mi, tile]}")


def whole_case(name):
    c = BY_NAME[name]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        got = pair_on_gpu(sc, c)
    slots, halves = check_pairing(c, got)
    check_legacy(c, got)
    assert halves == [] and 2 * len(slots) == len(c["stream"])
    return got


@pytest.mark.parametrize("name", names(K.shard_cases()) + ["region_cap_1"])
def test_shards(name):
    """chunks in their own regions, all in the last, a region full to its last word, single events, a run from region 5 to region 2,
    and eight random deals: the records depend on the events, never on where they lie"""
    got = whole_case(name)
    assert len(got["runs"]) == (32 if name == "region_cap_1" else 38)


def test_clamp():
    """region 0's counter says region_cap + 7: the first region_cap events pair cleanly, the raw counter is published, the compaction
    reports the overflow; the words behind the cap (motif 25) would raise PAIR_BAD_EVENT and table status 1 if they were read"""
    c = BY_NAME["clamp"]
    got = whole_case("clamp")
    assert got["published"][0] == c["region_cap"] + 7 and got["summary"] == c["region_cap"] and got["overflow"] == 1
    assert K.unpack(c["events"][c["region_cap"]])[1] == 25 and c["counters"][1] == 0


@pytest.mark.parametrize("name", names(K.seam_cases()))
def test_tile_seams(name):
    whole_case(name)


@pytest.mark.parametrize("name", names(K.prefix_cases()))
def test_prefix_sum_blocks(name):
    whole_case(name)


@pytest.mark.parametrize("name", names(K.carry_cases()))
def test_prefix_sum_carry(name):
    whole_case(name)


@pytest.mark.parametrize("name", names(K.grid_stride_cases()))
def test_grid_stride(name):
    whole_case(name)


def test_own_range_at_every_cut():
    """own_lo / own_hi on every run's START, START +- 1, END, END +- 1 (from the record's start, to its end, and windows seven cuts
    wide), the empty ranges and the whole record; then the largest pos_offset the record allows"""
    c = BY_NAME["own_shard_scrambled"]
    truth = K.shard_truth()
    ranges = K.own_ranges(truth, c["length"])
    off = 2 ** 31 - 1 - c["length"]
    kinds = set()
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        for own_lo, own_hi in ranges:
            own = (own_lo, own_hi, 0)
            slots, halves = check_pairing(c, pair_on_gpu(sc, c, own), own)
            kinds |= {h[3] for h in halves} | {s[3] for s in slots}
        for own_lo, own_hi in ((0, c["length"] + 1), (30000, 60000), (0, 49153), (49202, c["length"] + 1)):
            own = (own_lo, own_hi, off)
            slots, halves = check_pairing(c, pair_on_gpu(sc, c, own), own)
            assert max(max(r[0], r[1]) for r in slots + halves) <= 2 ** 31 - 1
        assert max(r[1] for r in slots + halves) == 2 ** 31 - 1                       # the run open to the end of the record
    assert kinds == {K.NOT_OWNED, 0, 1, 2, K.HALF_START, K.HALF_END, K.HALF_END + 1, K.HALF_END + 2}


def test_run_that_covers_the_own_range_leaves_no_half():
    c = BY_NAME["run_covers_own_range"]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        got = pair_on_gpu(sc, c)
    slots, halves = check_pairing(c, got)
    at = [r[:3] for r in K.shard_truth()].index((20000, 40000, 7))
    assert slots[at] == (0, 0, 0, K.NOT_OWNED) and all(h[2] != 7 for h in halves)


def test_two_halves_for_every_motif_fill_the_halves_buffer():
    c = BY_NAME["two_halves_per_motif"]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        got = pair_on_gpu(sc, c)
    slots, halves = check_pairing(c, got)
    check_legacy(c, got)
    assert got["n_halves"] == len(halves) == 2 * c["nm"] == 38 and [s for s in slots if s[3] != K.NOT_OWNED] == [(1200, 1300, 9, 0)]


@pytest.mark.parametrize("name", names(K.malformed_cases()))
def test_malformed_across_shards(name):
    """the flag and a normal return; the legacy table's status beside it (bit 0 malformed event, bit 1 two chunks for one entry)"""
    c = BY_NAME[name]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        got = pair_on_gpu(sc, c)
    if c["flags"] == K.DUP_CHUNK:
        assert got["flags"] & K.DUP_CHUNK, got["flags"]              # (which chunk the table keeps, and so what else is seen, is open)
    else:
        assert got["flags"] == c["flags"]
    assert np.array_equal(got["published"], c["counters"])
    dense, summary, overflow, _, status = legacy(name)
    assert status == {"dup_chunk_in_two_shards": 2, "motif_outside_the_launch_in_shard_1": 1}.get(name, 0)
    assert (got["summary"], got["overflow"], got["table_status"]) == (summary, overflow, status)
    assert np.array_equal(got["dense"], dense)


def test_hook_checks_its_arguments_and_respects_the_callers_capacities():
    c = BY_NAME["region_cap_1"]
    with ribbit_amd.Scanner(c["m_lo"], c["m_hi"]) as sc:
        out = ribbit_amd.DebugPairing()                                 # no buffers: nothing but the words may be written
        call = lambda region_cap, length, own_lo, own_hi: sc._L.ribbit_hip_debug_pair_events_sharded(
            sc._h, c["events"].ctypes.data, c["counters"].ctypes.data, region_cap, length, own_lo, own_hi, 0, C.byref(out))
        for bad in ((0, c["length"], 0, 5), ((1 << 18) + 1, c["length"], 0, 5), (1, -1, 0, 5), (1, c["length"], -1, 5), (1, c["length"], 5, 4)):
            assert call(*bad) == -1, bad                                # RIBBIT_E_ARG, before anything is read
        assert call(1, c["length"], 0, 2 ** 63 - 1) == 0
        assert list(out.status) == [0, 32, 0] and list(out.published) == [1] * 64 and (out.summary, out.overflow, out.table_status) == (64, 0, 0)
