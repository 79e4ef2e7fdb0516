"""The row outputs interleaved on one handle.  Best, classes, compounds, interruptions and nearest stage their inputs through one
pair of buffers, and every row output carves its intermediate arrays, its result on the device and its scans' and sorts'
temporary storage from one device work buffer (RowBufs in ribbit_amd/csrc/api_internal.h, the layouts in kernels.h), so that
buffer grows inside another feature than the one that sized it last; the results come up into pinned buffers of their own, "valid
until the handle's next same call, load or close" (include/ribbit_hip.h).  The four callers of the in-silico PCR's site search
share the site lists and the batch size besides.  Every answer here is compared with the host twin's."""
import ctypes as C

import numpy as np
import pytest

import interruptions_contract as ic
import primer_genome_contract as pg
import primer_specific_contract as ps
import primers_contract as pc
import ribbit_amd
from classes_contract import random_motif

pytestmark = pytest.mark.gpu


def _seq(n, seed=0):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def _rows(n, length, seed):
    """n rows of a record of `length` bases with everything a row output takes: intervals, motifs, labels, motif lengths, CIGARs"""
    rs = np.random.RandomState(seed)
    cigars = [ic.random_cigar(rs, int(k)) for k in rs.randint(0, 4, n)]
    starts = rs.randint(-20, length + 20, n)
    iv = np.stack([starts, starts + [ic.query_of(c) + (0 if rs.randint(5) else 1) for c in cigars]], 1).astype(np.int32)
    motifs = [random_motif(rs, int(k)) for k in rs.randint(1, 9, n)]
    return dict(iv=iv, motifs=motifs, labels=rs.randint(-2, 3, n), ks=np.array([len(m) for m in motifs]), cigars=cigars)


def _plain(result):
    return tuple(x if isinstance(x, (bytes, int, dict)) else x.tobytes() for x in (result if isinstance(result, tuple) else (result,)))


# name -> (the call on the handle, its host twin); each takes the record's bases and one _rows
CALLS = {
    "best": (lambda sc, seq, r: sc.record_best(r["iv"]), lambda seq, r: ribbit_amd.host_record_best(len(seq), r["iv"])),
    "classes": (lambda sc, seq, r: sc.record_classes(r["iv"], r["motifs"]), lambda seq, r: ribbit_amd.host_record_classes(len(seq), r["iv"], r["motifs"])),
    "compounds": (lambda sc, seq, r: sc.record_compounds(r["iv"], r["labels"], 40), lambda seq, r: ribbit_amd.host_record_compounds(len(seq), r["iv"], r["labels"], 40)),
    "interruptions": (lambda sc, seq, r: sc.record_interruptions(r["iv"], r["ks"], r["cigars"]),
                      lambda seq, r: ribbit_amd.host_record_interruptions(seq, r["iv"], r["ks"], r["cigars"])),
    "loci": (lambda sc, seq, r: sc.record_loci(r["iv"], 25), lambda seq, r: ribbit_amd.host_record_loci(len(seq), r["iv"], 25)),
    "overlap": (lambda sc, seq, r: sc.record_overlap(r["iv"], r["iv"][::3] + 7), lambda seq, r: ribbit_amd.host_record_overlap(len(seq), r["iv"], r["iv"][::3] + 7)),
    "repeats": (lambda sc, seq, r: sc.repeat_sequences("chr", r["iv"], 30), lambda seq, r: ribbit_amd.host_repeat_sequences("chr", seq, r["iv"], 30)),
    "nearest": (lambda sc, seq, r: sc.record_nearest(r["iv"], r["iv"][::3] + 7), lambda seq, r: ribbit_amd.host_record_nearest(len(seq), r["iv"], r["iv"][::3] + 7)),
    "composition": (lambda sc, seq, r: sc.record_composition(r["iv"], 30), lambda seq, r: ribbit_amd.host_record_composition(seq, r["iv"], 30)),
    "base windows": (lambda sc, seq, r: sc.record_base_windows(100), lambda seq, r: ribbit_amd.host_record_base_windows(seq, 100)),
    "density": (lambda sc, seq, r: sc.record_density(r["iv"], 100), lambda seq, r: ribbit_amd.host_record_density(len(seq), r["iv"], 100)),
    "mask": (lambda sc, seq, r: sc.mask_record(r["iv"], "soft", 60), lambda seq, r: ribbit_amd.host_mask_record(seq, r["iv"], "soft", 60)),
}


def _same(sc, seq, name, rows):
    on_handle, twin = CALLS[name]
    got, want = _plain(on_handle(sc, seq, rows)), _plain(twin(seq, rows))
    assert got == want, (name, len(rows["iv"]), len(seq))
    return got


def test_row_outputs_interleaved_on_one_handle():
    """the shared staging and work buffer are allocated by best at 70 rows, grow inside classes at 3 000, serve the other
    outputs at 300 and best again at 3 000.  Then every output at 1 row and at 65 (one lane past a wavefront: every region of the
    work buffer ends off its alignment).  Then the first call again, a shorter record, and the round in reverse"""
    few, mid, many = _rows(70, 3000, 1), _rows(300, 3000, 2), _rows(3000, 3000, 3)
    one, odd = _rows(1, 3000, 5), _rows(65, 3000, 6)
    steps = [("best", few), ("classes", many)] + [(name, mid) for name in ("compounds", "interruptions", "loci", "overlap", "repeats")] + [("best", many)]
    steps += [(name, mid) for name in ("nearest", "composition", "base windows", "density", "mask")]
    steps += [(name, rows) for rows in (one, odd) for name in CALLS]
    with ribbit_amd.Scanner(2, 30) as sc:
        seq = _seq(3000)
        sc.load_record(seq)
        answers = [_same(sc, seq, name, rows) for name, rows in steps]
        assert _same(sc, seq, *steps[0]) == answers[0]
        short = _seq(900, 1)
        sc.load_record(short)
        for name, rows in reversed(steps):
            _same(sc, short, name, rows)
        sc.load_record(seq)
        assert [_same(sc, seq, name, rows) for name, rows in steps] == answers


def test_the_work_buffer_regrows_inside_another_output_than_the_one_that_sized_it():
    """on a fresh handle best at 70 rows allocates the work buffer (a few KB: a buffer only ever grows, so nothing larger may have
    run before); nearest at 9 000 queries against 3 000 targets needs some 340 KB (96 KB of keys, 24 KB of orders, 216 KB of
    result) and so replaces it in the middle of the handle's life; best at 70 rows then carves the larger buffer and answers as before"""
    few, dense = _rows(70, 3000, 1), _rows(9000, 3000, 7)
    with ribbit_amd.Scanner(2, 30) as sc:
        seq = _seq(3000)
        sc.load_record(seq)
        first = _same(sc, seq, "best", few)
        _same(sc, seq, "nearest", dense)
        assert _same(sc, seq, "best", few) == first


def test_a_result_outlives_the_other_row_outputs():
    """what ribbit_hip_record_best returned is still there, byte for byte, after classes, compounds and interruptions on the same
    handle; what ribbit_hip_record_classes returned, after best; what ribbit_hip_record_nearest and ribbit_hip_record_composition
    returned, whose results on the device are regions of the work buffer the others carve anew, after best, classes and compounds"""
    L = ribbit_amd.load_library()
    seq = _seq(3000)
    r = _rows(3000, 3000, 4)
    iv = r["iv"]
    pool, off = "".join(r["motifs"]).encode(), np.concatenate([[0], np.cumsum(r["ks"])]).astype(np.int32)
    params = ribbit_amd.ScanParams()
    L.ribbit_scan_params_default(C.byref(params), 2, 30)
    h = C.c_void_p()
    assert L.ribbit_hip_open(C.byref(params), 0, C.byref(h)) == 0
    try:
        assert L.ribbit_hip_load_record(h, seq, len(seq)) == 0
        targets = np.ascontiguousarray(iv[::3] + 7)
        near, comp = C.c_void_p(), C.c_void_p()
        assert L.ribbit_hip_record_nearest(h, iv.ctypes.data, len(iv), targets.ctypes.data, len(targets), C.byref(near)) == 0
        assert L.ribbit_hip_record_composition(h, iv.ctypes.data, len(iv), 30, C.byref(comp)) == 0

        def rows_now():
            return (C.string_at(near.value, len(iv) * ribbit_amd.NEAREST_DT.itemsize), C.string_at(comp.value, len(iv) * ribbit_amd.COMPOSITION_DT.itemsize))

        kept_rows = rows_now()
        assert kept_rows == (ribbit_amd.host_record_nearest(len(seq), iv, targets).tobytes(), ribbit_amd.host_record_composition(seq, iv, 30).tobytes())
        best, n_best, bases = C.c_void_p(), C.c_size_t(), C.c_int64()
        assert L.ribbit_hip_record_best(h, iv.ctypes.data, len(iv), C.byref(best), C.byref(n_best), C.byref(bases)) == 0
        assert n_best.value > 10
        kept = C.string_at(best.value, 4 * n_best.value)
        want, _ = ribbit_amd.host_record_best(len(seq), iv)
        assert kept == want.tobytes()

        classes, strands, groups, n_groups = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        assert L.ribbit_hip_record_classes(h, iv.ctypes.data, len(iv), pool, off.ctypes.data, C.byref(classes), C.byref(strands), C.byref(groups), C.byref(n_groups)) == 0
        labels = np.ascontiguousarray(r["labels"], dtype=np.int32)
        chains, n_chains, members, n_members = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        assert L.ribbit_hip_record_compounds(h, iv.ctypes.data, labels.ctypes.data, len(iv), 40, C.byref(chains), C.byref(n_chains), C.byref(members), C.byref(n_members)) == 0
        ks, cigars = r["ks"].astype(np.int32), b"".join(r["cigars"])
        cigar_off = np.concatenate([[0], np.cumsum([len(c) for c in r["cigars"]])]).astype(np.int32)
        rows, sites, n_sites, observed, observed_off = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_void_p()
        assert L.ribbit_hip_record_interruptions(h, iv.ctypes.data, ks.ctypes.data, len(iv), cigars, cigar_off.ctypes.data, C.byref(rows), C.byref(sites),
                                                 C.byref(n_sites), C.byref(observed), C.byref(observed_off)) == 0
        assert n_chains.value > 0 and n_sites.value > 0
        assert C.string_at(best.value, 4 * n_best.value) == kept
        assert rows_now() == kept_rows

        def classes_now():
            return (C.string_at(classes.value, int(off[-1])), C.string_at(strands.value, len(iv)),
                    C.string_at(groups.value, n_groups.value * ribbit_amd.MOTIF_CLASS_DT.itemsize))

        kept_classes = classes_now()
        host = ribbit_amd.host_record_classes(len(seq), iv, pool, off)
        assert kept_classes == (host[0], host[1], host[2].tobytes())
        fewer = np.ascontiguousarray(iv[::-1][:2000])
        assert L.ribbit_hip_record_best(h, fewer.ctypes.data, len(fewer), C.byref(best), C.byref(n_best), C.byref(bases)) == 0
        assert classes_now() == kept_classes
        assert C.string_at(best.value, 4 * n_best.value) == ribbit_amd.host_record_best(len(seq), fewer)[0].tobytes()
    finally:
        L.ribbit_hip_close(h)


# ---- the four callers of the site search (api_primer_products.cpp: search_sites) on one handle: they share the work buffer, the
# site lists, the header's pinned words, the debug batch size and the code that sizes them
def _bytes(result):
    return tuple(np.ascontiguousarray(a).tobytes() for a in (result if isinstance(result, tuple) else (result,)))


def _search_call(sc, seq, name, k):
    """one call on the handle, which has `seq` loaded, at the batch size it names; -> its answer, which is its host twin's"""
    what, batch = name
    sc.debug_set_specific_batch(batch)
    if what == "specific":
        got, want = sc.record_specific_primer_pairs([], k["targets"]), ribbit_amd.host_record_specific_primer_pairs(seq, [], k["targets"])
        k.setdefault("pairs", got[0].copy())
    elif what == "products":
        got, want = sc.record_primer_products(k["pairs"]), ribbit_amd.host_record_primer_products(seq, k["pairs"])
    elif what == "shortlists":
        got, want = sc.record_primer_shortlists([], k["targets"]), ribbit_amd.host_record_primer_shortlists(seq, [], k["targets"])
        k.setdefault("lists", got.copy())
    elif what == "verdicts":
        got, want = sc.record_shortlist_verdicts(k["lists"], k["home"]), ribbit_amd.host_record_shortlist_verdicts(seq, k["lists"], k["home"])
    elif what == "amplicons":
        motifs = ["CA"] * len(k["pairs"])
        got, want = sc.record_pair_amplicons(k["pairs"], motifs, k["home"]), ribbit_amd.host_record_pair_amplicons(seq, k["pairs"], motifs, k["home"])
    else:
        got, want = sc.record_oligo_sites(k["oligos"]), ribbit_amd.host_record_oligo_sites(seq, k["oligos"])
    assert _bytes(got) == _bytes(want), (name, k["home"])
    return got


def test_the_site_search_callers_interleaved_on_one_handle():
    """the specific pairs at batch 1 size the site lists by one target; the products of the chosen pairs, with more oligos than a
    target has, grow them inside another caller; the verdicts with all targets in one batch grow them again; the amplicons at batch
    5 and two oligos' sites follow, and the first call again answers as before.  Then a foreign record, the home record again and
    the round in reverse.  Target 0 is primer_specific_contract's pinned one, so no answer is an empty one"""
    home = ps.constructed()["best pair copied"][0]
    foreign = pg.pinned_genomes()["best pair copied to the other record"][1]
    targets = [ps.TARGET] + pc.random_targets(len(home), np.random.RandomState(3), 12, longest=60).tolist()
    k = dict(targets=targets, home=1, oligos=[home[1304:1326].decode(), home[1613:1635].decode()])
    steps = [("specific", 1), ("products", 1), ("shortlists", 0), ("verdicts", 0), ("amplicons", 5), ("sites", 5), ("specific", 5)]
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(home)
        answers = [_search_call(sc, home, name, k) for name in steps]
        first = [_bytes(a) for a in answers]
        assert first[6] == first[0]
        sc.load_record(foreign)
        k["home"] = 0
        abroad = [_search_call(sc, foreign, name, k) for name in (("verdicts", 0), ("amplicons", 5), ("products", 5))]
        sc.load_record(home)
        k["home"] = 1
        assert [_bytes(_search_call(sc, home, name, k)) for name in reversed(steps)] == first[::-1]
    (pairs, products, specific), verdicts = answers[0], abroad[0]
    assert len(np.unique(k["pairs"][["left_start", "right_start"]][k["pairs"]["left_start"] >= 0])) > 8      # more than 16 oligos in the products' call
    assert ps.as_tuples(specific[:1])[0][:6] == ps.PINNED["best pair copied"][0] == (2, 44, 26, 0, 18, 2)
    assert (int(pairs["left_start"][0]), int(pairs["right_start"][0])) == (1304, 1613)
    assert bin(int(verdicts["other"][0])).count("1") == pg.PINNED["best pair copied to the other record"][0][4] == 14
    for p in (products[0], answers[1][0]):      # the chosen pair's products, from the specific pairs and from the products' own call
        assert p["own"] == 1 and p["products"] - p["own"] == 0
