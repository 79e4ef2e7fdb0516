#!/usr/bin/env python3
"""Timing of the primer pairs typed on a large record (GPU box; DESIGN.md section 25 quotes the figures).

  python3 tools/amplicons_timing.py random BASES [CALLS]   the chromosome-1-shaped simulated record of bench.py cut to BASES bases
        with its background made random (simulate.with_random_background): section 22's record, every flank unique
  python3 tools/amplicons_timing.py tiled BASES [CALLS]    the record as it is: every flank recurs at every locus

The generator's loci are the rows and the targets, each with its motif; Scanner.record_primer_pairs gives their pairs at flank
200.  Scanner.record_pair_amplicons and, beside it in the same session, Scanner.record_primer_products are called CALLS times
each (4 by default), alternating, at the default parameters: wall time per call, copies down and up and the synchronises
included.  The second is section 22's call and the yardstick for what the placing and the tract add.  Under
`rocprofv3 --kernel-trace --stats` the trace has pair_amplicons_kernel and amplicon_tracts_kernel beside site_scan_kernel.

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
    motifs = [motif.upper() for *_, motif in truth]
    made_s = time.perf_counter() - t0
    with ribbit_amd.Scanner(2, 100) as sc:
        sc.load_record(seq)
        pairs = sc.record_primer_pairs(rows, rows)
        pool = "".join(motifs).encode()
        offsets = np.concatenate([[0], np.cumsum([len(m) for m in motifs])]).astype(np.int32)
        amplicon_ms, product_ms = [], []
        for _ in range(calls):
            t0 = time.perf_counter()
            got = sc.record_pair_amplicons(pairs, (pool, offsets), 0)
            amplicon_ms.append(round(1e3 * (time.perf_counter() - t0), 2))
            t0 = time.perf_counter()
            products = sc.record_primer_products(pairs)
            product_ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    have = pairs["left_start"] >= 0
    assert np.array_equal(got["products"], products["products"]) and np.array_equal(got["left_forward"], products["left_forward"])
    one = got["products"] == 1
    tract = got["tract_end"] - got["tract_start"]
    some = np.flatnonzero(have)[:: max(1, int(have.sum()) // 40)][:40] if bases <= 20_000_000 else np.zeros(0, np.int64)
    if len(some):
        assert np.array_equal(ribbit_amd.host_record_pair_amplicons(seq, pairs[some], [motifs[i] for i in some], 0), got[some])
    return {"mode": mode, "bases": len(seq), "rows": len(rows), "pairs": int(have.sum()), "record_made_s": round(made_s, 1),
            "record_pair_amplicons_wall_ms": amplicon_ms, "record_primer_products_wall_ms": product_ms,
            "pairs_with_one_product": int(one.sum()), "pairs_with_more": int((got["products"] > 1).sum()), "pairs_over": int((got["products"] < 0).sum()),
            "pairs_with_a_tract": int((got["tract_start"] >= 0).sum()), "tracts_on_strand_1": int(got["tract_strand"].sum()),
            "mean_inner_part": round(float((got["inner_end"] - got["inner_start"])[one].mean()), 1) if one.any() else 0,
            "mean_tract": round(float(tract[got["tract_start"] >= 0].mean()), 1) if (got["tract_start"] >= 0).any() else 0,
            "first_product_is_the_designed_one": int((one & (got["start"] == pairs["left_start"]) & (got["end"] - got["start"] == pairs["product"])).sum()),
            "host_twin_pairs_compared": len(some)}


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 4)))
