#!/usr/bin/env python3
"""Timing of the shortlists' verdicts on a large record (GPU box; DESIGN.md section 24 quotes the figures).

  python3 tools/primer_genome_timing.py random BASES [CALLS]   the chromosome-1-shaped simulated record of bench.py cut to BASES
        bases with its background made random (simulate.with_random_background): the typical case, every flank unique
  python3 tools/primer_genome_timing.py tiled BASES [CALLS]    the record as it is, one fixed unit tiled between the loci: the
        worst case, every flank recurs at every locus and thousands of primers are the same oligo

Either way the generator's loci are the rows and the targets.  Scanner.record_primer_shortlists is called 1 + CALLS times (3 by
default) and then Scanner.record_shortlist_verdicts, as home and as a foreign record, at the default parameters; the first call of
each is left out: wall time per call (copies down and up and the synchronises included).  Beside them, in the same session and on
the same targets, Scanner.record_specific_primer_pairs: the yardstick, which makes the lists and judges them in one call.  Then
lists -> verdicts (home) -> choose is compared with that call, and the pairs are counted by outcome.  Under
`rocprofv3 --kernel-trace --stats` the trace has the kernels of one session.

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


def _timed(calls, f):
    ms, out = [], None
    for _ in range(1 + calls):
        t0 = time.perf_counter()
        out = f()
        ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    return ms, out


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
        lists_ms, lists = _timed(calls, lambda: sc.record_primer_shortlists(rows, rows))
        home_ms, home = _timed(calls, lambda: sc.record_shortlist_verdicts(lists, 1))
        foreign_ms, foreign = _timed(calls, lambda: sc.record_shortlist_verdicts(lists, 0))
        specific_ms, want = _timed(calls, lambda: sc.record_specific_primer_pairs(rows, rows))
    t0 = time.perf_counter()
    got = ribbit_amd.primer_shortlists_choose(lists, home)
    choose_ms = round(1e3 * (time.perf_counter() - t0), 2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    assert not foreign["own"].any() and np.array_equal(foreign["other"], home["other"] | home["own"])
    bits = lambda a: int(sum(bin(int(v)).count("1") for v in a))
    return {"mode": mode, "bases": len(seq), "targets": len(rows), "record_made_s": round(made_s, 1),
            "first_shortlists_wall_ms": lists_ms[0], "record_primer_shortlists_wall_ms": lists_ms[1:],
            "first_verdicts_wall_ms": home_ms[0], "record_shortlist_verdicts_home_wall_ms": home_ms[1:], "record_shortlist_verdicts_foreign_wall_ms": foreign_ms[1:],
            "first_specific_wall_ms": specific_ms[0], "record_specific_primer_pairs_wall_ms": specific_ms[1:], "primer_shortlists_choose_host_ms": choose_ms,
            "held_places": int((lists["left"]["start"] >= 0).sum() + (lists["right"]["start"] >= 0).sum()),
            "pairs_admissible": bits(home["admissible"]), "pairs_over": bits(home["over"]), "pairs_other_at_home": bits(home["other"]), "pairs_own": bits(home["own"]),
            "pairs_other_as_foreign": bits(foreign["other"])}


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)))
