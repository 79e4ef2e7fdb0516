"""Merged loci and the density track on the GPU (loci.hip through ribbit_hip_record_loci / ribbit_hip_record_density):
Scanner.record_loci and Scanner.record_density against the host twins and the numpy statement of the contract
(tests/loci_contract.py), and ribbit-hip --loci-bed / --density-bedgraph end to end."""
import functools
import types

import numpy as np
import pytest

import loci_contract
import ribbit_amd
import segments
from cli_rows import records, rows_by_record, run as _run, stages as _stages, write_nine_records
from mask_contract import masked_body
from repeat_contract import repeat_entries
from ribbit_amd.simulate import simulate_sequence, write_fasta

pytestmark = pytest.mark.gpu
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
GAPS = (0, 1, 5, 1000, I32_MAX)


def _seq(n, seed):
    return np.frombuffer(b"ACGTNacgt", np.uint8)[np.random.RandomState(seed).randint(0, 9, n)].tobytes()


def windows_for(length):
    return sorted({w for w in (1, 2, 31, 32, 33, 64, 1000, length - 1, length, length + 1, I32_MAX) if w >= 1})


def _same_loci(sc, length, iv, gap):
    got = sc.record_loci(iv, gap)
    assert got.dtype == ribbit_amd.LOCUS_DT
    assert got.tolist() == ribbit_amd.host_record_loci(length, iv, gap).tolist(), (length, gap)
    assert got.tolist() == loci_contract.record_loci(length, iv, gap), (length, gap)
    return got


def _same_density(sc, length, iv, window):
    got = sc.record_density(iv, window)
    assert got.dtype == np.int32
    assert got.tolist() == ribbit_amd.host_record_density(length, iv, window).tolist(), (length, window)
    assert got.tolist() == loci_contract.record_density(length, iv, window), (length, window)
    return got


def test_edge_cases_match_host_twin_and_contract():
    with ribbit_amd.Scanner(2, 30) as sc:
        for length in (0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 32 * 9 + 5, 2048, 4100):
            sc.load_record(_seq(length, length + 1))
            sets = [[], [(0, 1)], [(0, length)], [(3, 9), (5, 20)], [(-5, 4), (length - 2, length + 50)], [(I32_MIN, I32_MAX)],
                    [(50, 10), (20, 20), (90, -5)], [(50, 10), (10, 50), (20, 20), (200, 220), (90, -5)],
                    [(20, 30)] * 5 + [(100, 130)] * 3, [(10, 200), (20, 190), (30, 180), (40, 170), (50, 60), (10, 200)],
                    [(10, 20), (20, 30), (30, 31), (40, 50)], [(100, 130), (90, 120), (110, 140), (95, 100)],
                    [(length - 1, length)], [(length, length + 1)], [(-1, 0)]]
            for k in (1, 2, 4, 8) if length in (32 * 9 + 5, 2048, 4100) else ():
                sets.append([(32 * k - 1, 32 * k + 1), (32 * k, 32 * k + 33), (32 * k + 1, 32 * k + 2)])
                for s in (32 * k - 1, 32 * k, 32 * k + 1):
                    for e in (s + 1, 32 * k + 31, 32 * k + 32, 32 * k + 33):
                        sets.append([(s, e)])
                        sets.append([(0, s), (e, length)])
            for gap in GAPS:       # gaps of exactly gap and gap + 1
                d = min(gap, 1000)
                sets.append([(10, 20), (20 + d, 40 + d), (41 + 2 * d, 60 + 2 * d), (length - 9, length)])
            for n, iv in enumerate(sets):
                for gap in GAPS if n % 4 == 0 else (0, 5):
                    _same_loci(sc, length, iv, gap)
                for w in windows_for(length) if n % 4 == 0 else (1, 32, 33, 1000):
                    _same_density(sc, length, iv, w)


def test_ties_go_to_the_lowest_index_whatever_the_order():
    rows = [(100, 130), (90, 120), (110, 140), (95, 100), (300, 310), (301, 311), (299, 309), (302, 303)]
    rs = np.random.RandomState(3)
    with ribbit_amd.Scanner(2, 30) as sc:
        sc.load_record(_seq(400, 1))
        assert _same_loci(sc, 400, rows, 0)["best_row"].tolist() == [0, 4]
        for _ in range(20):
            _same_loci(sc, 400, [rows[i] for i in rs.permutation(len(rows))], 0)


def test_random_records():
    rs = np.random.RandomState(77)
    with ribbit_amd.Scanner(2, 30) as sc:
        for t in range(40):
            length = int(rs.randint(1000, 40_000))
            sc.load_record(_seq(length, t))
            n = int(rs.randint(0, 400))
            starts = rs.randint(-100, length + 100, n)
            iv = np.stack([starts, starts + rs.randint(-20, 3000 if t % 2 else 60, n)], 1)
            gap = int(rs.choice(GAPS))
            window = int(rs.choice(windows_for(length)))
            loci = _same_loci(sc, length, iv, gap)
            density = _same_density(sc, length, iv, window)
            assert loci["covered"].sum() == density.sum() == masked_body(b"A" * length, iv, "hard", 0).count(b"N")


def test_eight_megabase_record_with_its_bed_rows():
    seq = segments.simulated_record(8_000_000, 500)
    length = len(seq)
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        rows = ribbit_amd.bed_intervals(sc.refine_bed("chr"))
        assert len(rows) > 50_000
        giants = np.array([[1_000_003, 1_013_000], [2_500_000, 2_620_001], [7_990_000, 8_100_000]], np.int32)
        iv = np.concatenate([rows, giants])
        iv = iv[np.random.RandomState(1).permutation(len(iv))]
        third = rows[: len(rows) // 3]
        # the mask before and after on the same handle: the bitmap is shared, and is the one of the rows of each call
        assert sc.mask_record(third, "hard", 0) == masked_body(seq, third, "hard", 0)
        loci = _same_loci(sc, length, iv, 0)
        assert len(loci) < len(iv) and loci["rows"].sum() == len(iv) and loci["rows"].max() >= 2
        density = _same_density(sc, length, iv, 10_000)
        assert density.sum() == loci["covered"].sum()
        assert sc.mask_record(iv, "soft", 60) == masked_body(seq, iv, "soft", 60)
        _same_density(sc, length, iv, 100_000)
        # the same handle again, another gap, another window, a third of the rows: nothing of the first call may show through
        assert len(_same_loci(sc, length, iv, 50)) < len(loci)
        _same_density(sc, length, iv, 333)
        fewer = _same_loci(sc, length, third, 7)
        assert fewer["rows"].sum() == len(third)
        _same_density(sc, length, third, 2048)
        _same_density(sc, length, third, 2047)
        assert sc.mask_record(third, "soft", 80) == masked_body(seq, third, "soft", 80)
        assert _same_loci(sc, length, [], 0).shape == (0,)
        assert not _same_density(sc, length, [], 1_000_000).any()


def test_before_load_is_a_state_error():
    with ribbit_amd.Scanner(2, 30) as sc:
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_loci([(0, 1)])
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -3"):
            sc.record_density([(0, 1)], 10)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            sc.record_loci([(0, 1)], -1)
        with pytest.raises(ribbit_amd.RibbitHipError, match="error -1"):
            sc.record_density([(0, 1)], 0)


def _expected(fa, bed, gap, window):
    """the loci file and the bedGraph: the contract applied to the BED per record, in input order"""
    by_name = rows_by_record(bed)
    loci_text, density_text = "", ""
    for name, bases in records(fa):
        rows = ribbit_amd.bed_intervals(by_name.get(name, ""))
        loci_text += loci_contract.loci_lines(name, by_name.get(name, ""), loci_contract.record_loci(len(bases), rows, gap))
        density_text += loci_contract.density_lines(name, len(bases), window, loci_contract.record_density(len(bases), rows, window))
    return loci_text, density_text


@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """the nine-record FASTA and a run without loci and density, once: its BED, masked FASTA and repeat FASTA, and the loci file and
    the bedGraph that the contract makes of that BED"""
    d = tmp_path_factory.mktemp("nine")
    fa = d / "in.fa"
    write_nine_records(fa, 300, 77)
    common = ["-i", fa, "-m", 2, "-M", 30]
    bed0, masked0, repeats0 = d / "plain.bed", d / "plain_masked.fa", d / "plain_repeats.fa"
    _run(common + ["-o", bed0, "--masked-fasta", masked0, "--repeat-fasta", repeats0, "--timing", d / "t0.json"])
    want_bed = bed0.read_text()
    assert "loci" not in _stages(d / "t0.json") and "density" not in _stages(d / "t0.json")
    assert len(want_bed.splitlines()) > 100
    return types.SimpleNamespace(fa=fa, common=common, want_bed=want_bed, masked0=masked0, repeats0=repeats0,
                                 expected=functools.lru_cache(None)(lambda gap, window: _expected(fa, want_bed, gap, window)))


def test_cli_loci_bed_and_density_bedgraph(nine, tmp_path):
    fa, common, want_bed, masked0, repeats0 = nine.fa, nine.common, nine.want_bed, nine.masked0, nine.repeats0
    runs = [(0, 10_000, []),
            (0, 10_000, ["--devices", "0,0", "--jobs", "2"]),
            (25, 1000, ["--loci-gap", "25", "--density-window", "1000"]),
            (0, 10_000, ["--masked-fasta", tmp_path / "masked.fa", "--repeat-fasta", tmp_path / "repeats.fa"])]
    for k, (gap, window, extra) in enumerate(runs):
        bed, loci, graph, timing = tmp_path / f"r{k}.bed", tmp_path / f"r{k}.loci.bed", tmp_path / f"r{k}.bedgraph", tmp_path / f"t{k + 1}.json"
        _run(common + ["-o", bed, "--loci-bed", loci, "--density-bedgraph", graph, "--timing", timing] + extra)
        assert bed.read_text() == want_bed
        want_loci, want_graph = nine.expected(gap, window)
        assert loci.read_text() == want_loci, (gap, extra)
        assert graph.read_text() == want_graph, (window, extra)
        assert 0 < len(want_loci.splitlines()) < len(want_bed.splitlines())
        assert "loci" in _stages(timing) and "density" in _stages(timing)
    assert (tmp_path / "masked.fa").read_bytes() == masked0.read_bytes()
    assert (tmp_path / "repeats.fa").read_bytes() == repeats0.read_bytes()
    # one of the two alone: only its key
    _run(common + ["-o", tmp_path / "only.bed", "--density-bedgraph", tmp_path / "only.bedgraph", "--timing", tmp_path / "t9.json"])
    assert "density" in _stages(tmp_path / "t9.json") and "loci" not in _stages(tmp_path / "t9.json")
    assert (tmp_path / "only.bedgraph").read_text() == nine.expected(0, 10_000)[1]


def test_cli_all_four_outputs_side_by_side(nine, tmp_path):
    """the four row outputs in one run, the records dealt over two handle sets with two in flight on each: every file as when it is
    written alone, and --timing names the six stages of every record and then the four outputs' in their order"""
    bed, masked, repeats, loci, graph = (tmp_path / n for n in ("out.bed", "masked.fa", "repeats.fa", "loci.bed", "out.bedgraph"))
    _run(nine.common + ["-o", bed, "--density-bedgraph", graph, "--loci-bed", loci, "--repeat-fasta", repeats, "--masked-fasta", masked,
                        "--timing", tmp_path / "t.json", "--devices", "0,0", "--jobs", "2"])
    assert bed.read_text() == nine.want_bed
    by_name = rows_by_record(nine.want_bed)
    rows = [(n, b, ribbit_amd.bed_intervals(by_name.get(n, ""))) for n, b in records(nine.fa)]
    assert masked.read_bytes() == nine.masked0.read_bytes() == b"".join(b">" + n.encode() + b"\n" + masked_body(b, iv, "soft", 60) for n, b, iv in rows)
    assert repeats.read_bytes() == nine.repeats0.read_bytes() == b"".join(repeat_entries(n, b, iv, 100) for n, b, iv in rows)
    want_loci, want_graph = nine.expected(0, 10_000)
    assert loci.read_text() == want_loci
    assert graph.read_text() == want_graph
    assert list(_stages(tmp_path / "t.json")) == ["load", "perfect", "substitutions", "anchored", "dispatch", "refine_and_bed",
                                                  "mask", "repeats", "loci", "density"]


def test_cli_record_refined_in_slices(tmp_path):
    """one record refined in slices over three handles: its loci and density are those of the union of all slices' rows"""
    recs = [("small", simulate_sequence(30_000, 11, 2, 30, lower_rate=0.2)[0]),
            ("big", simulate_sequence(400_000, 12, 2, 30, n_block_rate=0.2, lower_rate=0.2)[0])]
    fa, bed0, bed = tmp_path / "in.fa", tmp_path / "plain.bed", tmp_path / "out.bed"
    loci, graph = tmp_path / "out.loci.bed", tmp_path / "out.bedgraph"
    write_fasta(str(fa), recs)
    _run(["-i", fa, "-o", bed0, "-m", 2, "-M", 30])
    r = _run(["-i", fa, "-o", bed, "-m", 2, "-M", 30, "--devices", "0,0,0", "--loci-bed", loci, "--loci-gap", "10", "--density-bedgraph", graph,
              "--density-window", "5000"], env={"RIBBIT_SHARD_MIN_SEEDS": "100", "RIBBIT_PROFILE": "1"})
    assert "[devices] refinement of big:" in r.stderr and "seeds in 3 slices" in r.stderr, r.stderr[-1500:]
    assert bed.read_text() == bed0.read_text()
    want_loci, want_graph = _expected(fa, bed0.read_text(), 10, 5000)
    assert loci.read_text() == want_loci
    assert graph.read_text() == want_graph
    assert sum(l.startswith("big\t") for l in want_loci.splitlines()) > 10
