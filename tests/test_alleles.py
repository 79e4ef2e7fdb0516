"""The markers' alleles over many samples, without a GPU: the plain statement of the contract (tests/alleles_contract.py) against the
pinned values, ribbit_host_marker_alleles against it on seeded random matrices and on every refusal, a sample's cells from hand-made
amplicons, both texts byte for byte, and the binding's new names."""
import inspect
from fractions import Fraction

import numpy as np
import pytest

import alleles_contract as alc
import amplicons_contract as ac
import primer_products_contract as prc
import ribbit_amd

DT, PAIRS_DT, AMPLICONS_DT = ribbit_amd.ALLELES_DT, ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PAIR_AMPLICONS_DT
INT32_MAX = 2**31 - 1


def as_tuples(rows):
    return [tuple(int(v) for v in r) for r in rows.tolist()]


def _twin(cells, designed, motif_lengths):
    rows = ribbit_amd.host_marker_alleles(np.asarray(cells, dtype=np.int64), designed, motif_lengths)
    assert rows.dtype == DT and DT.names == alc.FIELDS and DT.itemsize == 64
    return as_tuples(rows)


def test_the_contract_reproduces_the_pinned_table():
    assert sorted(alc.PINNED) == list("ABCDEF")
    for name, (cells, designed, m, want, text) in alc.PINNED.items():
        got = alc.marker(cells, designed, m)
        assert got == want, name
        if text and text[0] != ".":
            t = got[0]
            assert (alc.four_decimals(Fraction(got[12], t**2)), alc.four_decimals(Fraction(got[13], t**4))) == text, name
    # the two rounding cases: .5546875 and .703125 are no ties, .00005 is one and goes up
    assert Fraction(142, 256) == Fraction(5546875, 10**7) and Fraction(180, 256) == Fraction(703125, 10**6)
    assert alc.four_decimals(Fraction(1, 20000)) == "0.0001" and alc.four_decimals(Fraction(49999, 10**9)) == "0.0000" and alc.four_decimals(Fraction(1)) == "1.0000"


def test_the_pinned_values_from_the_twin():
    for name, (cells, designed, m, want, _) in alc.PINNED.items():
        assert _twin([[c] for c in cells], [designed], [m]) == [want], name
    # all of them side by side in one matrix of seven samples, the short ones filled up with absent cells
    names = list("ABCDEF")
    S = max(len(alc.PINNED[k][0]) for k in names)
    matrix = [[(alc.PINNED[k][0] + (0,) * S)[s] for k in names] for s in range(S)]
    want = alc.marker_alleles(matrix, [alc.PINNED[k][1] for k in names], [2] * 6)
    assert _twin(matrix, [alc.PINNED[k][1] for k in names], [2] * 6) == want
    assert [w[0] for w in want] == [4, 2, 4, 4, 0, 0] and want[1][1] == S - 2


def random_matrix(rs, S, n, kind):
    """-> (cells as S rows, designed, motif lengths): the sizes of a marker from few values, from many, or with ties for the most
    frequent one; one marker in eight without a pair; statuses mixed in; one size of 2^31 - 1"""
    designed = [int(rs.randint(80, 400)) if rs.randint(8) else int(rs.randint(-3, 1)) for _ in range(n)]
    steps = [int(rs.randint(1, 9)) for _ in range(n)]
    cells = np.zeros((S, n), dtype=np.int64)
    for i in range(n):
        d, m = max(designed[i], 100), steps[i]
        if kind == "few":
            column = d + m * rs.randint(-2, 2, S)
        elif kind == "many":
            column = d + rs.randint(-60, 61, S)
        else:      # ties: every size as often as the others, as far as S allows
            column = d + m * (np.arange(S) % int(rs.randint(1, 5)))
            rs.shuffle(column)
        status = rs.random_sample(S)
        column = np.where(status < 0.1, 0, np.where(status < 0.15, -1, np.where(status < 0.2, -2, column)))
        cells[:, i] = column
    if n:
        cells[rs.randint(S), rs.randint(n)] = INT32_MAX
    return cells.tolist(), designed, steps


@pytest.mark.parametrize("kind", ["few", "many", "ties"])
def test_random_matrices_equal_the_contract(kind):
    rs = np.random.RandomState({"few": 11, "many": 12, "ties": 13}[kind])
    seen_tie = seen_max = 0
    for S in list(range(1, 41)):
        n = int(rs.randint(1, 12))
        cells, designed, steps = random_matrix(rs, S, n, kind)
        want = alc.marker_alleles(cells, designed, steps)
        assert _twin(cells, designed, steps) == want, (kind, S)
        for i, w in enumerate(want):
            column = [row[i] for row in cells if row[i] > 0]
            seen_tie += w[0] > 0 and sum(1 for a in set(column) if column.count(a) == w[8]) > 1
            seen_max += w[6] == INT32_MAX
            if designed[i] > 0:
                assert sum(w[:4]) == S and 0 <= w[12] <= w[0] ** 2 and 0 <= w[13] <= w[12] * w[0] ** 2
    assert seen_max >= 10 and (kind != "ties" or seen_tie >= 20)


def test_no_markers_and_one_cell():
    assert _twin([[]], [], []) == [] and _twin([[], [], []], [], []) == []
    assert _twin([[7]], [7], [3]) == [(1, 0, 0, 0, 1, 7, 7, 7, 1, 1, 0, 0, 0, 0)]
    assert _twin([[INT32_MAX], [1]], [1], [INT32_MAX]) == [alc.marker([INT32_MAX, 1], 1, INT32_MAX)]
    # 1024 samples, all of another size: t^4 = 2^40
    cells = [[100 + s] for s in range(1024)]
    assert _twin(cells, [100], [1]) == [(1024, 0, 0, 0, 1024, 100, 1123, 100, 1, 1, 0, 0, 1024**2 - 1024, 1024**4 - 1024**3 - 1024**2 + 1024)]


def test_every_refusal_of_the_twin():
    label = "ribbit_host_marker_alleles error -1: "
    cells = [[100, 102, 0], [-2, -1, 104]]
    for bad, at in (((1, 2), -3), ((0, 0), -2**31)):
        spoiled = [list(r) for r in cells]
        spoiled[bad[0]][bad[1]] = at
        with pytest.raises(alc.Refused) as e:
            alc.marker_alleles(spoiled, [100] * 3, [2] * 3)
        index = bad[0] * 3 + bad[1]
        assert e.value.index == index
        with pytest.raises(ribbit_amd.RibbitHipError, match=label + rf"cell {index} \(sample {bad[0]}, marker {bad[1]}\) is {at}, below -2"):
            _twin(spoiled, [100] * 3, [2] * 3)
    for steps, index in (([2, 0, 2], 1), ([-1, 2, 0], 0), ([1, 1, -2**31], 2)):
        with pytest.raises(alc.Refused) as e:
            alc.marker_alleles(cells, [100] * 3, steps)
        assert e.value.index == index
        with pytest.raises(ribbit_amd.RibbitHipError, match=label + f"marker {index}: a motif length of {steps[index]}, below 1"):
            _twin(cells, [100] * 3, steps)
    # the motif length is asked of a row without a pair too, and before the cells
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "marker 2: a motif length of 0, below 1"):
        _twin([[-5, 0, 0]], [100, 100, -1], [2, 2, 0])
    with pytest.raises(alc.Refused):
        alc.marker_alleles([], [], [])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "0 samples, not 1 .. 1024"):
        ribbit_amd.host_marker_alleles(np.zeros((0, 2), np.int32), [100, 100], [2, 2])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "1025 samples, not 1 .. 1024"):
        ribbit_amd.host_marker_alleles(np.zeros((1025, 1), np.int32), [100], [2])
    assert len(ribbit_amd.host_marker_alleles(np.zeros((1024, 1), np.int32), [100], [2])) == 1
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + r"16777217 markers \(at most 16777216\)"):
        ribbit_amd.host_marker_alleles(np.zeros((1, (1 << 24) + 1), np.int32), np.zeros((1 << 24) + 1, np.int32), np.ones((1 << 24) + 1, np.int32))
    with pytest.raises(ValueError, match="the cells are a matrix, one row per sample"):
        ribbit_amd.host_marker_alleles([1, 2, 3], [100], [2])
    with pytest.raises(ValueError, match="3 markers, 2 designed products and 3 motif lengths"):
        ribbit_amd.host_marker_alleles(cells, [100] * 2, [2] * 3)
    with pytest.raises(ValueError, match="a cell is not an int32"):
        ribbit_amd.host_marker_alleles([[1 << 31]], [100], [2])


def _amplicon(products, start=-1, end=-1):
    placed = (0, start, end, 0, 1, start + 18, end - 18, -1, -1, 0, 0) if products > 0 else ac.NONE
    return (1, 0, 0, 1, products) + placed


def test_the_cells_of_hand_made_amplicons():
    made = [_amplicon(1, 40, 165), _amplicon(0), _amplicon(2, 7, 90), _amplicon(INT32_MAX, 7, 90), _amplicon(-1), ac.NO_PAIR, _amplicon(1, 0, INT32_MAX)]
    has_pair = [True] * 5 + [False, True]
    want = [125, 0, -1, -1, -2, 0, INT32_MAX]
    assert [alc.cell_of(a, h) for a, h in zip(made, has_pair)] == want
    got = ribbit_amd.pair_amplicon_sizes(np.array(made, dtype=AMPLICONS_DT))
    assert got.dtype == np.int32 and got.tolist() == want
    assert ribbit_amd.pair_amplicon_sizes(np.zeros(0, dtype=AMPLICONS_DT)).tolist() == []
    # what the merge leaves is what the cells are made of: one product in each of two records are two
    both = ribbit_amd.pair_amplicons_merge(np.array(made[:1], dtype=AMPLICONS_DT), np.array(made[:1], dtype=AMPLICONS_DT))
    assert ribbit_amd.pair_amplicon_sizes(both).tolist() == [-1]
    label = "ribbit_pair_amplicon_sizes error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 1: products -2 is below -1"):
        ribbit_amd.pair_amplicon_sizes(np.array([made[0], _amplicon(-2)], dtype=AMPLICONS_DT))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 0: a product from 9 to 9"):
        ribbit_amd.pair_amplicon_sizes(np.array([_amplicon(1, 9, 9)], dtype=AMPLICONS_DT))


def bed_line(k, motif="CA", name="home\twith a tab"):
    return "\t".join([name, str(100 * k), str(100 * k + 20), motif, ".", ".", "10", ".", ".", ".", "20M"])


def _text_case():
    names = list("ABCDE") + ["F"]
    pairs = []
    for k, name in enumerate(names):
        row = list(prc.pair_tuple(ac.A, ac.B, 10 + k, 10 + k + alc.PINNED[name][1] - len(ac.B) if name != "F" else 0))
        row[2], row[8], row[14] = 601, -5, max(alc.PINNED[name][1], 0)
        pairs.append(tuple(row) if name != "F" else ac_no_pair())
    S = 7
    matrix = [[(alc.PINNED[k][0] + (0,) * S)[s] for k in names] for s in range(S)]
    designed = [alc.PINNED[k][1] for k in names]
    bed = "".join(bed_line(k) + "\n" for k in range(len(names)))
    return bed, pairs, matrix, designed, S


def ac_no_pair():
    return (-1, 0, 0, 0, 0, 0) * 2 + (0,) * 20


def test_the_alleles_text():
    bed, pairs, matrix, designed, S = _text_case()
    rows = alc.marker_alleles(matrix, designed, [2] * 6)
    got = ribbit_amd.bed_alleles_text(bed, np.array(pairs, dtype=PAIRS_DT), np.array(rows, dtype=DT), S).decode()
    assert got == alc.alleles_lines(bed, pairs, rows, S)
    lines = [l.split("\t") for l in got.splitlines()]
    assert all(len(c) == 2 + 11 + 23 - 1 for c in lines)      # (the name holds a tab: 34 columns)
    assert [c[-2:] for c in lines] == [["0.0000", "0.0000"], ["0.5000", "0.3750"], ["0.6250", "0.5547"], ["0.7500", "0.7031"], [".", "."], [".", "."]]
    assert lines[2][-14:-2] == ["7", "4", "1", "1", "1", "3", "100", "105", "102", "2", "1", "1"]
    assert lines[4][-14:-2] == ["7", "0", "7", "0", "0", "0", ".", ".", ".", "0", "0", "0"] and lines[5][-23:] == ["."] * 23
    assert lines[0][12:21] == ["10", "28", ac.A, "60.1", "92", "110", ac.B, "-0.5", "100"]
    assert all(l.startswith(bed_line(k) + "\t") for k, l in enumerate(got.splitlines()))
    # a last line without its newline; nothing at all
    assert ribbit_amd.bed_alleles_text(bed[:-1], np.array(pairs, dtype=PAIRS_DT), np.array(rows, dtype=DT), S).decode() == got
    assert ribbit_amd.bed_alleles_text("", np.zeros(0, dtype=PAIRS_DT), np.zeros(0, dtype=DT), 3) == b""
    # 1024 samples of as many sizes: the denominators are 2^20 and 2^40
    wide = alc.marker([100 + s for s in range(1024)], 100, 1)
    one = ribbit_amd.bed_alleles_text(bed_line(0), np.array(pairs[:1], dtype=PAIRS_DT), np.array([wide], dtype=DT), 1024).decode()
    assert one == alc.alleles_lines(bed_line(0), pairs[:1], [wide], 1024) and one.endswith("\t0.9990\t0.9990\n")
    label = "ribbit_bed_alleles_text error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "the BED text has 6 lines, not the 2 of the rows"):
        ribbit_amd.bed_alleles_text(bed, np.array(pairs[:2], dtype=PAIRS_DT), np.array(rows[:2], dtype=DT), S)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "row 0: 4 typed cells of 3 samples"):
        ribbit_amd.bed_alleles_text(bed, np.array(pairs, dtype=PAIRS_DT), np.array(rows, dtype=DT), 3)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "0 samples, not 1 .. 1024"):
        ribbit_amd.bed_alleles_text(bed, np.array(pairs, dtype=PAIRS_DT), np.array(rows, dtype=DT), 0)
    long = np.array(pairs, dtype=PAIRS_DT)
    long["left_length"][3] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "row 3: a primer of 33 bases, not 1 .. 32"):
        ribbit_amd.bed_alleles_text(bed, long, np.array(rows, dtype=DT), S)
    with pytest.raises(ValueError, match="6 pairs and 5 records of alleles"):
        ribbit_amd.bed_alleles_text(bed, np.array(pairs, dtype=PAIRS_DT), np.array(rows[:5], dtype=DT), S)


def test_the_matrix_text():
    bed, _, matrix, designed, S = _text_case()
    names = [f"sample {s}" for s in range(S)]
    got = ribbit_amd.allele_matrix_text(bed, matrix, designed, names).decode()
    assert got == alc.matrix_lines(bed, matrix, designed, names)
    lines = got.splitlines()
    assert lines[0] == "#name\tstart\tend\tmotif\tdesigned\t" + "\t".join(names)
    assert lines[3] == "home\twith a tab\t200\t220\tCA\t100\t100\t102\t102\t105\t.\t+\t*"
    assert lines[6] == "home\twith a tab\t500\t520\tCA\t.\t100\t102\t.\t+\t.\t.\t."
    assert ribbit_amd.allele_matrix_text(bed[:-1], matrix, designed, names).decode() == got
    assert ribbit_amd.allele_matrix_text("", np.zeros((2, 0), np.int32), [], ["a", "b"]) == b"#name\tstart\tend\tmotif\tdesigned\ta\tb\n"
    big = ribbit_amd.allele_matrix_text(bed_line(0), [[INT32_MAX]], [INT32_MAX], ["s"]).decode()
    assert big.splitlines()[1].endswith(f"\tCA\t{INT32_MAX}\t{INT32_MAX}")
    label = "ribbit_allele_matrix_text error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "the BED text has 6 lines, not the 1 of the rows"):
        ribbit_amd.allele_matrix_text(bed, [[100]], [100], ["s"])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "line 1 of the BED text is not a row"):
        ribbit_amd.allele_matrix_text(bed_line(0) + "\na\tb\tc\n", [[100, 100]], [100, 100], ["s"])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + r"cell 3 \(sample 1, marker 1\) is -3, below -2"):
        ribbit_amd.allele_matrix_text(bed_line(0) + "\n" + bed_line(1), [[100, 100], [0, -3]], [100, 100], ["s", "t"])
    with pytest.raises(ValueError, match="2 samples and 1 names"):
        ribbit_amd.allele_matrix_text(bed_line(0), [[100], [100]], [100], ["s"])


def test_names_sizes_and_the_binding():
    for name in ("ALLELES_DT", "pair_amplicon_sizes", "host_marker_alleles", "bed_alleles_text", "allele_matrix_text"):
        assert name in ribbit_amd.__all__ and hasattr(ribbit_amd, name)
    for symbol in ("ribbit_pair_amplicon_sizes", "ribbit_hip_marker_alleles", "ribbit_host_marker_alleles", "ribbit_alleles_free", "ribbit_bed_alleles_text",
                   "ribbit_allele_matrix_text"):
        assert symbol in ribbit_amd.ABI_SYMBOLS and hasattr(ribbit_amd.load_library(), symbol)
    assert str(inspect.signature(ribbit_amd.host_marker_alleles)) == "(cells, designed, motif_lengths) -> 'np.ndarray'"
    assert str(inspect.signature(ribbit_amd.Scanner.marker_alleles)) == "(self, cells, designed, motif_lengths) -> 'np.ndarray'"
    assert str(inspect.signature(ribbit_amd.pair_amplicon_sizes)) == "(amplicons) -> 'np.ndarray'"
    assert str(inspect.signature(ribbit_amd.bed_alleles_text)) == "(bed, pairs, rows, n_samples: 'int') -> 'bytes'"
    assert str(inspect.signature(ribbit_amd.allele_matrix_text)) == "(bed, cells, designed, names) -> 'bytes'"
    assert DT.itemsize == 64 and DT.fields["het_num"][1] == 48 and DT.fields["pic_num"][1] == 56
    assert ribbit_amd.load_library().ribbit_hip_abi_version() == 1
    L = ribbit_amd.load_library()
    assert L.ribbit_hip_marker_alleles(None, None, 1, 0, None, None, None) == -1 and b"null handle" in L.ribbit_hip_last_error()
