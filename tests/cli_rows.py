"""What the end-to-end tests of ribbit-hip's row outputs share (test_mask_gpu.py, test_repeat_fasta_gpu.py, test_loci_gpu.py):
running the tool, its --timing stages, the BED rows of each record, and the FASTA with nine records of every kind."""
import json
import os
import subprocess

import ribbit_amd
from ribbit_amd.simulate import simulate_sequence, write_fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")


def rows_by_record(bed: str):
    out = {}
    for line in bed.splitlines(keepends=True):
        out.setdefault(line.split("\t")[0], []).append(line)
    return {k: "".join(v) for k, v in out.items()}


def records(fa):
    """the records the tool writes row outputs for: all but a nameless empty one"""
    return [(n, b) for n, b, last in ribbit_amd.read_fasta(str(fa)) if n or b]


def run(args, env=None, timeout=600):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def stages(path):
    return json.loads(path.read_text())["stage_ms_summed_over_records"]


def write_nine_records(fa, seed, lead_seed):
    """six simulated records of 20-65 kb with their descriptions, one that vanishes (a header without bases between two others), an
    empty last one, and a nameless body before the first header"""
    recs = []
    for k in range(6):
        s, _ = simulate_sequence(20_000 + 9_000 * k, seed + k, 2, 30, n_block_rate=0.3, lower_rate=0.2)
        recs.append((f"rec{k} description dropped", s))
    write_fasta(str(fa), recs[:3] + [("vanishes", b"")] + recs[3:] + [("empty_last", b"")], width=70)
    lead, _ = simulate_sequence(15_000, lead_seed, 2, 30, lower_rate=0.3)
    with open(fa, "rb") as f:
        body = f.read()
    with open(fa, "wb") as f:            # a nameless body before the first header
        f.write(b"".join(lead[i:i + 50] + b"\n" for i in range(0, len(lead), 50)) + body)
    names = [n for n, _, _ in ribbit_amd.read_fasta(str(fa))]
    assert names[0] == "" and names[-1] == "empty_last" and "vanishes" not in names
