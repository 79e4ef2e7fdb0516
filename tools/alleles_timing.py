#!/usr/bin/env python3
"""Times ribbit_hip_marker_alleles on a random genotype matrix: the kernel and the copy down by HIP events (the library prints both
with RIBBIT_PROFILE set; the copy is the host's strided gather into the staging buffer and the transfer), the whole call by the wall
clock, which ends behind the stream's synchronise, and the host twin for scale.
    python tools/alleles_timing.py [--shapes 1000000x8,1000000x64,1000000x1024] [--out profiles/NAME.json]
A shape is markers x samples.  Every shape runs in a child process of its own with its own time limit; a child that fails ends the
run.  The device's records are compared with the twin's, byte for byte, at every shape."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_matrix(n, S, seed):
    """n markers of 80 .. 399 bases designed, motifs of 1 .. 8; a sample's size is the designed one -2 .. +2 units off, one cell in
    twenty is absent, several or over; one marker in 16 has no pair.  At most 64 rows are drawn: more samples repeat them."""
    rs = np.random.RandomState(seed)
    designed = rs.randint(80, 400, n).astype(np.int32)
    steps = rs.randint(1, 9, n).astype(np.int32)
    drawn = min(S, 64)
    cells = np.empty((S, n), dtype=np.int32)
    for s in range(drawn):
        row = designed + steps * rs.randint(-2, 3, n).astype(np.int32)
        status = rs.randint(0, 60, n)
        cells[s] = np.where(status < 3, -status.astype(np.int32), row)
    for s in range(drawn, S):
        cells[s] = cells[s % drawn]
    designed[::16] = 0
    return cells, designed, steps


def one(n, S):
    import ribbit_amd
    cells, designed, steps = random_matrix(n, S, 1)
    result = {"markers": n, "samples": S, "cells": n * S}
    t0 = time.perf_counter()
    want = ribbit_amd.host_marker_alleles(cells, designed, steps)
    result["host_twin_s"] = time.perf_counter() - t0
    with ribbit_amd.Scanner(2, 6) as sc:
        got = sc.marker_alleles(cells, designed, steps)      # (the first call loads the code object and sizes the buffers)
        result["equals_twin"] = got.tobytes() == want.tobytes()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = sc.marker_alleles(cells, designed, steps)
            walls.append(time.perf_counter() - t0)
    has = designed > 0
    result.update(wall_s=walls, alleles_mean=float(got["alleles"][has].mean()), typed_mean=float(got["typed"][has].mean()))
    # what moves per cell: 4 bytes gathered on the host into the staging buffer, 4 over the bus, 4 read by the kernel; per marker 8
    # bytes of designed product and motif length down, and a record of 64 bytes written by the kernel and brought back
    result["bytes_per_cell"] = 4 + (8 + 64) / S
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000x8,1000000x64,1000000x1024")
    ap.add_argument("--limit", type=int, default=400, help="seconds a shape may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", default="")
    args = ap.parse_args()
    if args.one:
        n, S = (int(v) for v in args.one.split("x"))
        return one(n, S)
    results = []
    for shape in args.shapes.split(","):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape], capture_output=True, text=True, timeout=args.limit,
                               env=dict(os.environ, RIBBIT_PROFILE="1"))
        if child.returncode != 0:
            sys.exit(f"{shape}: exit status {child.returncode}\n{child.stderr[-2000:]}")
        result = json.loads(child.stdout.strip().splitlines()[-1])
        if not result["equals_twin"]:
            sys.exit(f"{shape}: the device's records differ from the twin's")
        calls = [m.groupdict() for m in re.finditer(r"\[alleles\] markers (?P<markers>\d+) samples (?P<samples>\d+) batch (?P<batch>\d+) copy_ms (?P<copy_ms>[\d.]+) kernel_ms (?P<kernel_ms>[\d.]+)",
                                                    child.stderr)]
        result["batch_markers"] = int(calls[-1]["batch"])
        result["device_ms"] = [{"copy_ms": float(c["copy_ms"]), "kernel_ms": float(c["kernel_ms"])} for c in calls[1:]]      # (without the warm-up call)
        results.append(result)
        print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "ribbit_hip_marker_alleles on a random genotype matrix, markers x samples (tools/alleles_timing.py), MI355X", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
