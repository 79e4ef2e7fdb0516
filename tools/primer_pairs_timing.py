#!/usr/bin/env python3
"""Timing of the primer pair output on a chromosome-sized record (GPU box; DESIGN.md section 21 quotes the figures).

  python3 tools/primer_pairs_timing.py cli WORKDIR [BASES]      the chromosome-1-sized simulated record of bench.py through
        ribbit-hip --best-bed --composition-bed --primer-bed --primer-pair-bed --timing, twice: the wall time of the
        `primer_pairs` stage beside `primers`, `best` and `composition`; the rows that get a pair, and those whose pair is not
        --primer-bed's two primers; leaves WORKDIR/in.fa and WORKDIR/out.bed for the other mode
  python3 tools/primer_pairs_timing.py call WORKDIR [TARGETS]   the same record and rows through Scanner.record_primer_pairs at
        flank 200: the best selection's rows as targets (the first TARGETS of them, 1,000,000 by default) against all rows, five
        calls, wall time per call (copies down and up and the synchronise included).  Under `rocprofv3 --kernel-trace --stats`
        the trace has `primer_pairs_kernel` alone

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
STAGES = ("refine_and_bed", "best", "composition", "primers", "primer_pairs")


def cli(work: str, bases: int | None) -> dict:
    os.makedirs(work, exist_ok=True)
    fa, bed = os.path.join(work, "in.fa"), os.path.join(work, "out.bed")
    seq = grch38_shaped_record(0, bases, 2, 100)
    write_fasta(fa, [("chr1", seq)])
    runs = []
    for k in range(2):
        t0 = time.perf_counter()
        subprocess.run([BIN, "-i", fa, "-o", bed, "-m", "2", "-M", "100", "--best-bed", os.path.join(work, "best.bed"), "--composition-bed",
                        os.path.join(work, "composition.bed"), "--primer-bed", os.path.join(work, "primers.bed"), "--primer-pair-bed", os.path.join(work, "pairs.bed"),
                        "--timing", os.path.join(work, "timing.json")], check=True, stderr=subprocess.DEVNULL)
        wall = time.perf_counter() - t0
        stages = json.load(open(os.path.join(work, "timing.json")))["stage_ms_summed_over_records"]
        runs.append({"wall_s": round(wall, 3), "stage_ms": {k: round(stages[k], 1) for k in STAGES}})
    paired = differ = rows = 0
    with open(os.path.join(work, "pairs.bed")) as pairs, open(os.path.join(work, "primers.bed")) as primers:
        for pair_line, primer_line in zip(pairs, primers):
            rows += 1
            pair, alone = pair_line.split("\t")[-21:-12], primer_line.split("\t")[-11:-2]      # the eight primer columns and the product
            paired += pair[0] != "."
            differ += pair[0] != "." and pair != alone
    return {"mode": "cli", "bases": len(seq), "bed_rows": sum(1 for _ in open(bed)), "pair_rows": rows, "rows_with_a_pair": paired,
            "rows_whose_pair_is_not_primer_beds": differ, "primer_pair_bed_bytes": os.path.getsize(os.path.join(work, "pairs.bed")), "runs": runs}


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
            got = sc.record_primer_pairs(rows, targets)
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    some = targets[:: max(1, len(targets) // 2000)]
    t0 = time.perf_counter()
    twin = ribbit_amd.host_record_primer_pairs(seq, rows, some)
    twin_ms = 1e3 * (time.perf_counter() - t0)
    assert np.array_equal(twin, got[:: max(1, len(targets) // 2000)])
    have = got["left_start"] >= 0
    return {"mode": "call", "bases": len(seq), "rows": len(rows), "targets": len(targets), "flank": 200, "record_primer_pairs_wall_ms": ms,
            "targets_with_a_pair": int(have.sum()), "pairs_not_of_the_two_best": int((have & ((got["left_rank"] > 0) | (got["right_rank"] > 0))).sum()),
            "candidates_per_target": round(float((got["left_candidates"] + got["right_candidates"]).mean()), 1),
            "passing_per_target": round(float((got["left_passed"] + got["right_passed"]).mean()), 1),
            "admissible_pairs_per_target": round(float(got["pairs_admissible"].mean()), 1), "host_twin_targets": len(some), "host_twin_ms": round(twin_ms, 1)}


if __name__ == "__main__":
    mode, work = sys.argv[1], sys.argv[2]
    extra = int(sys.argv[3]) if len(sys.argv) > 3 else None
    print(json.dumps(cli(work, extra) if mode == "cli" else call(work, extra or 1_000_000)))
