#!/usr/bin/env python3
"""Timing of the in-silico PCR of primer pairs on a large record (GPU box; DESIGN.md section 22 quotes the figures).

  python3 tools/primer_products_timing.py random BASES [CALLS]   the chromosome-1-shaped simulated record of bench.py cut to BASES
        bases with its background made random (simulate.with_random_background): the typical case, every flank unique
  python3 tools/primer_products_timing.py tiled BASES [CALLS]    the record as it is, one fixed unit tiled between the loci: the
        worst case, every flank recurs at every locus and thousands of primers are the same oligo

Either way the generator's loci are the rows and the targets, Scanner.record_primer_pairs gives their pairs at flank 200, and
Scanner.record_primer_products is called CALLS times (3 by default) at the default parameters: wall time per call (copies down
and up and the synchronises included), the sites per oligo, the share of specific pairs, and the perfect scan's kernel time on
the same record, which reads the same planes for 99 periods: a yardstick, not a bound.  Under `rocprofv3 --kernel-trace --stats`
the trace has the new kernels beside scan_perfect_kernel.

Each run prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ribbit_amd  # noqa: E402
from ribbit_amd.simulate import grch38_shaped_record, simulate_sequence, with_random_background  # noqa: E402


def run(mode: str, bases: int, calls: int) -> dict:
    t0 = time.perf_counter()
    seq = grch38_shaped_record(0, bases, 2, 100)
    _, truth = simulate_sequence(bases, 4, 2, 100)      # (the loci of that record: its generator seed and motif range)
    if mode == "random":
        seq = with_random_background(seq, truth, 1)
    rows = np.array([(s, e) for s, e, *_ in truth], dtype=np.int32).reshape(-1, 2)
    made_s = time.perf_counter() - t0
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        sc.scan_perfect_runs(copy=False)
        perfect_ms = sc.timing_ms(1)      # RIBBIT_TIME_SCAN
        pairs = sc.record_primer_pairs(rows, rows)
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            got = sc.record_primer_products(pairs)
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    have = pairs["left_start"] >= 0
    counted = have & (got["products"] >= 0)
    sites = got["left_forward"].astype(np.int64) + got["left_reverse"] + got["right_forward"] + got["right_reverse"]
    oligos = {(int(r[f"{side}_length"]), int(r[f"{side}_bases_lo"]), int(r[f"{side}_bases_hi"])) for r in pairs[have][:: max(1, int(have.sum()) // 20000)]
              for side in ("left", "right")}
    some = np.flatnonzero(have)[:: max(1, int(have.sum()) // 40)][:40] if bases <= 20_000_000 else np.zeros(0, np.int64)
    if len(some):
        assert np.array_equal(ribbit_amd.host_record_primer_products(seq, pairs[some]), got[some])
    return {"mode": mode, "bases": len(seq), "rows": len(rows), "pairs": int(have.sum()), "record_made_s": round(made_s, 1),
            "record_primer_products_wall_ms": ms, "site_scan_bases_per_s_by_wall": round(len(seq) / (min(ms) * 1e-3)),
            "scan_perfect_kernel_ms": round(perfect_ms, 2), "sites_per_oligo": round(float(sites[have].mean()) / 2, 2),
            "longest_list": int(max(got[n][have].max() for n in ("left_forward", "left_reverse", "right_forward", "right_reverse"))) if have.any() else 0,
            "pairs_with_a_list_over_max_sites": int((have & (got["products"] < 0)).sum()),
            "specific_pairs": int((counted & (got["products"] - got["own"] == 0)).sum()), "pairs_without_their_own_product": int((counted & (got["own"] == 0)).sum()),
            "distinct_oligos_in_a_sample_of_pairs": [len(oligos), 2 * len(pairs[have][:: max(1, int(have.sum()) // 20000)])], "host_twin_pairs_compared": len(some)}


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)))
