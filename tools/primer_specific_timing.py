#!/usr/bin/env python3
"""Timing of the specific primer pairs on a large record (GPU box; DESIGN.md section 23 quotes the figures).

  python3 tools/primer_specific_timing.py random BASES [CALLS]   the chromosome-1-shaped simulated record of bench.py cut to BASES
        bases with its background made random (simulate.with_random_background): the typical case, every flank unique
  python3 tools/primer_specific_timing.py tiled BASES [CALLS]    the record as it is, one fixed unit tiled between the loci: the
        worst case, every flank recurs at every locus and thousands of primers are the same oligo

Either way the generator's loci are the rows and the targets.  Scanner.record_specific_primer_pairs is called 1 + CALLS times (3
by default) at the default parameters and the first call is left out: wall time per call (copies down and up and the synchronises
included).  Beside it, in the same session and on the same targets, Scanner.record_primer_pairs followed by
Scanner.record_primer_products, the two calls this one puts together for a single pair per target: the yardstick.  Then the share of
the targets by outcome (place 0, a later place, no pair) and the pairs by outcome.  Under `rocprofv3 --kernel-trace --stats` the
trace has the kernels of one session.

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
    ms, two_ms = [], []
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        for _ in range(1 + calls):
            t0 = time.perf_counter()
            pairs, products, specific = sc.record_specific_primer_pairs(rows, rows)
            ms.append(round(1e3 * (time.perf_counter() - t0), 2))
        for _ in range(1 + calls):
            t0 = time.perf_counter()
            best = sc.record_primer_pairs(rows, rows)
            best_products = sc.record_primer_products(best)
            two_ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    n = max(len(rows), 1)
    place = specific["place"]
    some = np.flatnonzero(specific["pairs_admissible"] > 0)
    some = some[:: max(1, len(some) // 24)][:24] if bases <= 20_000_000 else np.zeros(0, np.int64)
    if len(some):
        twin = ribbit_amd.host_record_specific_primer_pairs(seq, rows, rows[some])
        assert all(np.array_equal(a, b[some]) for a, b in zip(twin, (pairs, products, specific)))
    want = np.where(best_products["products"] < 0, -1, best_products["products"] - best_products["own"])
    assert np.array_equal(specific["first_products"], np.where(best["left_start"] >= 0, want, 0))
    return {"mode": mode, "bases": len(seq), "targets": len(rows), "record_made_s": round(made_s, 1),
            "first_call_wall_ms": ms[0], "record_specific_primer_pairs_wall_ms": ms[1:],
            "first_pairs_plus_products_wall_ms": two_ms[0], "record_primer_pairs_plus_record_primer_products_wall_ms": two_ms[1:],
            "targets_with_an_admissible_pair": int((specific["pairs_admissible"] > 0).sum()),
            "share_place_0": round(float((place == 0).sum()) / n, 4), "share_later_place": round(float((place > 0).sum()) / n, 4),
            "share_no_pair": round(float((place < 0).sum()) / n, 4), "latest_place": int(place.max()) if len(place) else -1,
            "pairs_admissible": int(specific["pairs_admissible"].sum()), "pairs_specific": int(specific["pairs_specific"].sum()),
            "pairs_over": int(specific["pairs_over"].sum()), "pairs_other": int(specific["pairs_other"].sum()), "host_twin_targets_compared": len(some)}


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)))
