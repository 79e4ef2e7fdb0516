#!/usr/bin/env python3
"""Timing of the primer output on a chromosome-sized record (GPU box; DESIGN.md section 20 quotes the figures).

  python3 tools/primers_timing.py cli WORKDIR [BASES]      the chromosome-1-sized simulated record of bench.py through
        ribbit-hip --best-bed --composition-bed --primer-bed --timing, twice: the wall time of the `primers` stage beside `best`
        and `composition`; leaves WORKDIR/in.fa and WORKDIR/out.bed for the other mode
  python3 tools/primers_timing.py call WORKDIR [TARGETS]   the same record and rows through Scanner.record_primers at flank 200:
        the best selection's rows as targets (the first TARGETS of them, 1,000,000 by default) against all rows, five calls, wall
        time per call (copies down and up and the synchronise included).  Under `rocprofv3 --kernel-trace --stats` the trace has
        `primers_kernel` alone

Each mode prints one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ribbit_amd  # noqa: E402
from ribbit_amd.simulate import grch38_shaped_record, write_fasta  # noqa: E402

BIN = os.path.join(ROOT, "ribbit_amd", "ribbit-hip")


def cli(work: str, bases: int | None) -> dict:
    os.makedirs(work, exist_ok=True)
    fa, bed = os.path.join(work, "in.fa"), os.path.join(work, "out.bed")
    seq = grch38_shaped_record(0, bases, 2, 100)
    write_fasta(fa, [("chr1", seq)])
    runs = []
    for k in range(2):
        t0 = time.perf_counter()
        subprocess.run([BIN, "-i", fa, "-o", bed, "-m", "2", "-M", "100", "--best-bed", os.path.join(work, "best.bed"), "--composition-bed",
                        os.path.join(work, "composition.bed"), "--primer-bed", os.path.join(work, "primers.bed"), "--timing", os.path.join(work, "timing.json")],
                       check=True, stderr=subprocess.DEVNULL)
        wall = time.perf_counter() - t0
        stages = json.load(open(os.path.join(work, "timing.json")))["stage_ms_summed_over_records"]
        runs.append({"wall_s": round(wall, 3), "stage_ms": {k: round(stages[k], 1) for k in ("refine_and_bed", "best", "composition", "primers")}})
    lines = open(os.path.join(work, "primers.bed")).read().splitlines()
    both = sum(line.rsplit("\t", 3)[1] != "." for line in lines)
    return {"mode": "cli", "bases": len(seq), "bed_rows": sum(1 for _ in open(bed)), "primer_rows": len(lines), "rows_with_both_primers": both,
            "primer_bed_bytes": os.path.getsize(os.path.join(work, "primers.bed")), "runs": runs}


def call(work: str, n_targets: int) -> dict:
    seq = ribbit_amd.read_fasta(os.path.join(work, "in.fa"))[0][1]
    rows = ribbit_amd.bed_intervals(open(os.path.join(work, "out.bed"), "rb").read())
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        best, _ = sc.record_best(rows)
        targets = np.ascontiguousarray(rows[best][:n_targets])
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            got = sc.record_primers(rows, targets)
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    some = targets[:: max(1, len(targets) // 2000)]
    t0 = time.perf_counter()
    twin = ribbit_amd.host_record_primers(seq, rows, some)
    twin_ms = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(twin, got[:: max(1, len(targets) // 2000)])
    return {"mode": "call", "bases": len(seq), "rows": len(rows), "targets": len(targets), "flank": 200, "record_primers_wall_ms": ms,
            "targets_with_both_primers": int(((got["left_start"] >= 0) & (got["right_start"] >= 0)).sum()),
            "candidates_per_target": round(float((got["left_candidates"] + got["right_candidates"]).mean()), 1),
            "host_twin_targets": len(some), "host_twin_ms": round(twin_ms, 1)}


if __name__ == "__main__":
    mode, work = sys.argv[1], sys.argv[2]
    extra = int(sys.argv[3]) if len(sys.argv) > 3 else None
    print(json.dumps(cli(work, extra) if mode == "cli" else call(work, extra or 1_000_000)))
