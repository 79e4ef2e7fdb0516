"""ribbit-hip's --population-list, --allele-bed and --allele-matrix up to the GPU: every usage error and every refusal of the list
file ends the run with status 1 and one line, before any output file is made and any GPU is touched."""
import subprocess

from cli_rows import BIN


def _dies(args, message):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, args
    assert r.stdout == ""
    assert r.stderr == "ribbit-hip: " + message + "\n", args


def test_the_options_need_each_other(tmp_path):
    a, m, l = tmp_path / "a.bed", tmp_path / "m.tsv", tmp_path / "list.tsv"
    _dies(["-i", "in.fa", "--population-list", l], "--population-list needs --allele-bed or --allele-matrix")
    _dies(["-i", "in.fa", "--allele-bed", a], "--allele-bed needs --population-list")
    _dies(["-i", "in.fa", "--allele-matrix", m], "--allele-matrix needs --population-list")
    _dies(["--allele-matrix=" + str(m), "--allele-bed=" + str(a), "-i", "in.fa"], "--allele-bed needs --population-list")
    for option in ("--population-list", "--allele-bed", "--allele-matrix"):
        _dies(["-i", "in.fa", option, ""], f"{option} wants a file name")
        _dies(["-i", "in.fa", option], f"the required argument for option '{option}' is missing")
    assert not a.exists() and not m.exists()


def test_every_refusal_of_the_list(tmp_path):
    a, l = tmp_path / "a.bed", tmp_path / "list.tsv"
    one, two = tmp_path / "one.fa", tmp_path / "two.fa"
    one.write_text(">r\nACGT\n")
    two.write_text(">r\nACGT\n")
    args = ["-i", "in.fa", "-o", tmp_path / "out.bed", "--allele-bed", a, "--population-list", l]
    _dies(args, f"--population-list: cannot open '{l}' for reading")
    where = lambda k: f"--population-list: line {k} of '{l}' "
    for text, message in (
            ("", f"--population-list: '{l}' names no sample"),
            ("# nobody\n\n\r\n#\tx\n", f"--population-list: '{l}' names no sample"),
            (f"s1\t{one}\nno tab here\n", where(2) + "is not name<TAB>path"),
            (f"# samples\n\ns1\t{one}\textra\n", where(3) + "has more than one tab (no name and no path may hold one)"),
            (f"s1\t{one}\n\t{two}\n", where(2) + "has an empty name"),
            (f"s1\t\n", where(1) + "has an empty path"),
            (f"s1\t{one}\n# between\ns2\t{two}\n\ns1\t{two}\n", where(5) + "names 's1' again (line 1 has it)"),
            (f"s1\t{one}\ns2\t{tmp_path / 'missing.fa'}\n", where(2) + f"names '{tmp_path / 'missing.fa'}', which cannot be opened for reading"),
            ("".join(f"s{k}\t{one}\n" for k in range(1025)), where(1025) + "is sample 1025 (at most 1024)"),
            ("#\n" + "".join(f"s{k}\t{one}\n" for k in range(1026)), where(1026) + "is sample 1025 (at most 1024)")):
        l.write_text(text)
        _dies(args, message)
    # nothing was made on the way: the list is read first
    assert not a.exists() and not (tmp_path / "out.bed").exists()
    # a good list of 1024 samples with Windows line ends: the outputs are opened next, still before the GPU
    l.write_bytes("".join(f"s{k}\t{one}\r\n" for k in range(1024)).encode())
    _dies(args[:-4] + ["--allele-bed", tmp_path / "missing" / "a.bed", "--population-list", l], f"--allele-bed: cannot open '{tmp_path / 'missing' / 'a.bed'}' for writing")
    _dies(args + ["--allele-matrix", tmp_path / "missing" / "m.tsv"], f"--allele-matrix: cannot open '{tmp_path / 'missing' / 'm.tsv'}' for writing")


def test_help_names_the_options():
    r = subprocess.run([BIN, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == ""
    at = [r.stderr.index(f"\n  {name} arg ") for name in ("--panel-max", "--population-list", "--allele-bed", "--allele-matrix", "--masked-fasta")]
    assert at == sorted(at)
    entry = " ".join(r.stderr[at[1]:at[2]].split())
    assert "name<TAB>path" in entry and "1 .. 1024 samples" in entry and "only if the list names it" in entry and "one int32 is kept per sample and row" in entry
    entry = " ".join(r.stderr[at[2]:at[3]].split())
    assert "23 columns" in entry and "He = 1 - sum p^2" in entry and "PIC" in entry and "typed (exactly one product), absent, several, over" in entry
    entry = " ".join(r.stderr[at[3]:at[4]].split())
    assert "'.' absent, '+' several, '*' over" in entry
