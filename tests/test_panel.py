"""The primer pairs pooled into multiplex panels, without a GPU: ribbit_host_panel_pools against the plain statement of the contract
(tests/panel_contract.py) on the pinned values and on seeded random panels, the properties every answer has, the panel text, every
refusal, the binding's new names, and ribbit-hip's three options up to the GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import panel_contract as pc
import ribbit_amd
from panel_cases import check_properties, random_panel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")
needs_tool = pytest.mark.skipif(not os.path.exists(BIN), reason="ribbit_amd/ribbit-hip is not built")
PAIRS_DT, DT = ribbit_amd.PRIMER_PAIRS_DT, ribbit_amd.PANEL_DT


def _twin(pairs, extra=None, **fields):
    rows, pools = ribbit_amd.host_panel_pools(np.array(pairs, dtype=PAIRS_DT), extra, ribbit_amd.panel_params(**fields))
    assert rows.dtype == DT and DT.names == pc.FIELDS and DT.itemsize == 32 and isinstance(pools, int)
    return pc.as_tuples(rows), pools


def test_the_pinned_values():
    cases = pc.pinned_cases()
    assert len(cases) == 13
    for name, case in cases.items():
        pairs, extra, fields, _, pools, _ = case
        assert pc.panel_pools(pairs, extra, pc.params(**fields)) == (pc.pinned_rows(case), pools), name
        assert _twin(pairs, extra, **fields) == (pc.pinned_rows(case), pools), name
    assert pc.duplex(pc.DIMER_A, pc.DIMER_B) == (10, 10)
    # index order would pool the star the other way round
    star = cases["star"]
    assert [r[0] for r in pc.pinned_rows(star)] == [1, 1, 1, 0]


def test_the_defaults():
    p = ribbit_amd.panel_params()
    assert {n: getattr(p, n) for n, _ in p._fields_} == pc.DEFAULTS
    assert ctypes.sizeof(p) == 20


RULES_OFF = (dict(), dict(max_cross_any=32, max_cross_end=32), dict(size_gap=0), dict(max_cross_product=0), dict(max_cross_any=4, max_cross_end=3),
             dict(max_cross_product=1 << 30, size_gap=100000))


@pytest.mark.parametrize("n,seed", [(60, 1), (33, 2), (9, 3)])
def test_random_panels_equal_the_contract(n, seed):
    rs = np.random.RandomState(seed)
    pairs, extra = random_panel(n, rs)
    met = set()
    for ex in (None, extra):
        for fields in RULES_OFF:
            for pool_size in (8, 3):
                want = pc.panel_pools(pairs, ex, pc.params(pool_size=pool_size, **fields))
                got = _twin(pairs, ex, pool_size=pool_size, **fields)
                assert got == want, (n, ex is None, fields, pool_size)
                check_properties(pairs, got[0], got[1], pool_size)
                for k, rule in enumerate(("dimer", "size", "near")):
                    if any(r[2 + k] for r in got[0]):
                        met.add((rule, tuple(sorted(fields.items()))))
    # every rule has refused something where it is on, and nothing where it is off
    assert {("dimer", ()), ("size", ()), ("near", ())} <= met
    assert ("dimer", (("max_cross_any", 32), ("max_cross_end", 32))) not in met
    assert ("size", (("size_gap", 0),)) not in met and ("near", (("max_cross_product", 0),)) not in met


def test_small_panels_and_pool_sizes():
    assert _twin([]) == ([], 0)
    q = [pc.quiet_pair(k, 5000 * k, 100 + 60 * k) for k in range(4)]
    assert _twin(q[:1]) == ([(0, 0, 0, 0, 0, 0, 0, 0)], 1)
    assert _twin([pc.NO_PAIR]) == ([pc.NOT_POOLED], 0)
    assert [r[0] for r in _twin(q, pool_size=65536)[0]] == [0, 0, 0, 0]
    assert [r[0] for r in _twin(q, pool_size=3)[0]] == [0, 0, 0, 1]
    assert [r[0] for r in _twin(q * 2, pool_size=2, size_gap=0)[0]] == [0, 0, 1, 1, 2, 2, 3, 3]
    # all in conflict by size: as many pools as pairs, in index order
    same = [pc.quiet_pair(k, 0, 200) for k in range(4)]
    assert _twin(same) == ([(k, 3, 0, 3, 0, 0, 0, 0) for k in range(4)], 4)
    # the span and the sizes are judged in 64 bits
    far = [pc.pair(pc.QUIET[0], pc.QUIET[1], 2**31 - 40, 2**31 - 20), pc.pair(pc.QUIET[2], pc.QUIET[3], 0, 50)]
    ex = [(0, -2**31, -2**31), (0, 2**31 - 1, 2**31 - 1)]
    assert _twin(far, ex, max_cross_product=1 << 30) == pc.panel_pools(far, ex, pc.params(max_cross_product=1 << 30)) == ([(0, 0, 0, 0, 0, 0, 0, 0)] * 2, 1)


def test_every_refusal_of_the_twin():
    label = "ribbit_host_panel_pools error -1: "
    q = [pc.quiet_pair(0, 0, 100), pc.quiet_pair(1, 0, 200)]
    for fields, message in ((dict(max_cross_any=-1), "max_cross_any -1 is outside 0 .. 32"), (dict(max_cross_any=33), "max_cross_any 33 is outside 0 .. 32"),
                            (dict(max_cross_end=-1), "max_cross_end -1 is outside 0 .. 32"), (dict(max_cross_end=33), "max_cross_end 33 is outside 0 .. 32"),
                            (dict(size_gap=-1), "size_gap -1 is outside 0 .. 100000"), (dict(size_gap=100001), "size_gap 100001 is outside 0 .. 100000"),
                            (dict(max_cross_product=-1), "max_cross_product -1 is outside 0 .. 1073741824"),
                            (dict(max_cross_product=(1 << 30) + 1), "max_cross_product 1073741825 is outside 0 .. 1073741824"),
                            (dict(pool_size=0), "pool_size 0 is outside 1 .. 65536"), (dict(pool_size=65537), "pool_size 65537 is outside 1 .. 65536")):
        with pytest.raises(ribbit_amd.RibbitHipError, match=label + message):
            _twin(q, **fields)
    for fields in (dict(max_cross_any=0, max_cross_end=0), dict(size_gap=100000, max_cross_product=1 << 30, pool_size=65536)):
        assert _twin(q, **fields)[1] >= 1
    bad = np.array(q, dtype=PAIRS_DT)
    bad["right_length"][1] = 33
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 1: a primer of 33 bases, not 1 .. 32"):
        ribbit_amd.host_panel_pools(bad)
    bad["right_length"][1], bad["left_length"][0] = 20, 0
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 0: a primer of 0 bases, not 1 .. 32"):
        ribbit_amd.host_panel_pools(bad)
    bad["left_start"][0] = -1      # (a row without a pair is not looked at)
    assert ribbit_amd.host_panel_pools(bad)[1] == 1
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 1: size_lo 201 is above size_hi 200"):
        _twin(q, [(0, 1, 1), (0, 201, 200)])
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "pair 0: group -2 is below -1"):
        _twin(q, [(-2, 1, 1), (0, 1, 1)])
    too_many = np.zeros(pc.MAX_PAIRS + 1, dtype=PAIRS_DT)
    too_many["left_start"] = -1
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + r"65537 pairs \(at most 65536\)"):
        ribbit_amd.host_panel_pools(too_many)
    assert ribbit_amd.host_panel_pools(too_many[:-1])[1] == 0
    with pytest.raises(ValueError, match="2 pairs want 6 extra values"):
        _twin(q, [(0, 1, 1)])
    with pytest.raises(ValueError, match="an extra value is not an int32"):
        _twin(q, [(0, 1, 1), (0, 1, 1 << 31)])
    with pytest.raises(TypeError):
        ribbit_amd.host_panel_pools(np.array(q, dtype=PAIRS_DT), None, ribbit_amd.product_params())


def test_panel_params_refuses_bad_fields():
    assert ribbit_amd.panel_params(pool_size=12).pool_size == 12 and ribbit_amd.panel_params(size_gap=-2**31).size_gap == -2**31
    with pytest.raises(TypeError) as e:
        ribbit_amd.panel_params(no_such_field=1)
    assert str(e.value) == "RibbitPanelParams has no field 'no_such_field'"
    for value in (2**31, -2**31 - 1):
        with pytest.raises(ValueError) as e:
            ribbit_amd.panel_params(pool_size=value)
        assert str(e.value) == f"pool_size {value} does not fit int32"


def marker_line(k, product):
    """a line as ribbit_bed_marker_text writes it, with a tab in the record's name"""
    return "\t".join([f"home\twith a tab", str(100 * k), str(100 * k + 20), "CA", ".", ".", "10", ".", ".", ".", "20M",
                      "5", "23", "ACGT", "60.0", "63", "81", "ACGT", "60.0", str(product), "1", "other", "0", "90", "+", "90", str(90 - product), ".", ".", ".", "."])


def test_the_text():
    products = [300, 120, 250, 120, 90, 120]
    text = "".join(marker_line(k, p) + "\n" for k, p in enumerate(products))
    rows = [(1, 4, 1, 2, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 0), pc.NOT_POOLED, (0, 2, 2, 0, 0, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0, 0), (0, 7, 3, 3, 3, 0, 0, 0)]
    got = ribbit_amd.bed_panel_text(text, np.array(rows, dtype=DT)).decode()
    assert got == pc.panel_lines(text, rows, products)
    lines = got.splitlines()
    assert [l.split("\t")[2] for l in lines] == ["100", "300", "500", "400", "0"]      # pool 0 by product then input order, then pool 1
    assert all(l.rsplit("\t", 5)[0] + "\n" in text for l in lines) and lines[0].endswith("\t0\t0\t0\t0\t0") and lines[-1].endswith("\t1\t4\t1\t2\t1")
    # a last line without its newline; no members; nothing at all
    assert ribbit_amd.bed_panel_text(text[:-1], np.array(rows, dtype=DT)).decode() == got
    assert ribbit_amd.bed_panel_text(text, np.array([pc.NOT_POOLED] * 6, dtype=DT)) == b""
    assert ribbit_amd.bed_panel_text("", np.zeros(0, dtype=DT)) == b""
    label = "ribbit_bed_panel_text error -1: "
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "the marker text has 6 lines, not the 2 of the rows"):
        ribbit_amd.bed_panel_text(text, np.array(rows[:2], dtype=DT))
    dotted = text.replace("60.0\t120\t", "60.0\t.\t", 1)      # (line 1's designed product)
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "line 1 of the marker text has no designed product"):
        ribbit_amd.bed_panel_text(dotted, np.array(rows, dtype=DT))
    with pytest.raises(ribbit_amd.RibbitHipError, match=label + "line 0 of the marker text has no designed product"):
        ribbit_amd.bed_panel_text("a\tb\tc\n", np.array(rows[:1], dtype=DT))
    assert ribbit_amd.bed_panel_text("a\tb\tc\n", np.array([pc.NOT_POOLED], dtype=DT)) == b""      # (only the members' lines are read)


def test_names_sizes_and_the_binding():
    for name in ("PANEL_DT", "PanelParams", "panel_params", "host_panel_pools", "bed_panel_text"):
        assert name in ribbit_amd.__all__ and hasattr(ribbit_amd, name)
    for symbol in ("ribbit_panel_params_default", "ribbit_hip_panel_pools", "ribbit_host_panel_pools", "ribbit_panel_free", "ribbit_hip_debug_panel_conflicts",
                   "ribbit_bed_panel_text"):
        assert symbol in ribbit_amd.ABI_SYMBOLS and hasattr(ribbit_amd.load_library(), symbol)
    assert str(inspect.signature(ribbit_amd.host_panel_pools)) == "(pairs, extra=None, params: 'PanelParams | None' = None)"
    assert str(inspect.signature(ribbit_amd.Scanner.panel_pools)) == "(self, pairs, extra=None, params: 'PanelParams | None' = None)"
    assert str(inspect.signature(ribbit_amd.Scanner.debug_panel_conflicts)) == "(self, pairs, extra=None, params: 'PanelParams | None' = None) -> 'np.ndarray'"
    assert str(inspect.signature(ribbit_amd.bed_panel_text)) == "(marker_text, rows) -> 'bytes'"
    assert str(inspect.signature(ribbit_amd.panel_params)) == "(**fields) -> 'PanelParams'"
    assert [f for f, _ in ribbit_amd.PanelParams._fields_] == ["max_cross_any", "max_cross_end", "size_gap", "max_cross_product", "pool_size"]
    assert DT.names == ("pool", "conflicts", "dimer", "size", "near", "reserved0", "reserved1", "reserved2")
    assert ribbit_amd.load_library().ribbit_hip_abi_version() == 1


# ---- the tool up to the GPU
def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


@needs_tool
def test_cli_the_panel_needs_the_markers(tmp_path):
    needs = "--panel-bed needs --marker-fasta and --marker-bed"
    _dies(["-i", "in.fa", "--panel-bed", tmp_path / "p.bed"], needs)
    _dies(["-i", "in.fa", "--panel-bed", tmp_path / "p.bed", "--marker-fasta", "o.fa"], needs)
    _dies(["--panel-bed=" + str(tmp_path / "p.bed"), "-i", "in.fa", "--marker-bed", tmp_path / "m.bed"], needs)
    assert not (tmp_path / "p.bed").exists() and not (tmp_path / "m.bed").exists()
    _dies(["-i", "in.fa", "--panel-bed", ""], "--panel-bed wants a file name")
    _dies(["-i", "in.fa", "--panel-bed"], "the required argument for option '--panel-bed' is missing")
    _dies(["-i", "in.fa", "--panel-pool-size", "4"], "--panel-pool-size needs --panel-bed")
    _dies(["-i", "in.fa", "--panel-max", "4"], "--panel-max needs --panel-bed")
    for option in ("--panel-pool-size", "--panel-max"):
        for value in ("0", "65537", "-1", "8x", "", "100000"):
            _dies(["-i", "in.fa", option, value], f"{option} wants a whole number (1 .. 65536), got '{value}'")
    # with everything given, the files are opened before the GPU is touched
    other = tmp_path / "other.fa"
    other.write_text(">a\nACGT\n")
    _dies(["-i", "in.fa", "--marker-fasta", other, "--marker-bed", tmp_path / "m.bed", "--panel-bed", tmp_path / "missing" / "p.bed", "--panel-pool-size", "65536",
           "--panel-max", "1"], f"--panel-bed: cannot open '{tmp_path / 'missing' / 'p.bed'}' for writing")


@needs_tool
def test_cli_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    at = [r.stderr.index(f"\n  {name} arg ") for name in ("--marker-bed", "--panel-bed", "--panel-pool-size", "--panel-max", "--masked-fasta")]
    assert at == sorted(at)
    entry = " ".join(r.stderr[at[1]:at[2]].split())
    assert "--marker-fasta and --marker-bed" in entry and "pool, conflicts, dimer, size, near" in entry and "low-numbered pools fill first" in entry
    assert "Default: 8" in r.stderr[at[2]:at[3]] and "Default: 16384" in r.stderr[at[3]:at[4]]
