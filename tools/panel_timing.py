#!/usr/bin/env python3
"""Times ribbit_hip_panel_pools on random admissible primer pairs: the three device stages by HIP events (the library prints them
with RIBBIT_PROFILE set), the whole call by the wall clock, and the host twin at the smallest size for scale.
    python tools/panel_timing.py [--sizes 4096,16384,65536] [--twin 4096] [--out profiles/NAME.json]
Every size runs in a child process of its own with its own time limit; a child that fails ends the run."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_pairs(n, seed):
    """n pairs of oligos of 18 .. 25 bases, GC 40 .. 60 %, a C or G at the 3' end, products of 80 .. 500 bases on 24 records"""
    import ribbit_amd
    rs = np.random.RandomState(seed)
    out = np.zeros(n, dtype=ribbit_amd.PRIMER_PAIRS_DT)
    extra = np.zeros((n, 3), dtype=np.int32)

    def oligo():
        while True:
            k = int(rs.randint(18, 26))
            codes = rs.randint(0, 4, k)
            gc = int(((codes == 1) | (codes == 2)).sum())
            if 40 * k <= 100 * gc <= 60 * k and codes[-1] in (1, 2):
                return codes

    for i in range(n):
        a, b = oligo(), oligo()
        forward_b = (3 - b)[::-1]      # the right primer's forward-strand bases
        start, product = int(rs.randint(0, 50_000_000)), int(rs.randint(80, 501))
        for side, codes, at in (("left", a, start), ("right", forward_b, start + product - len(b))):
            bases = sum(int(c) << (2 * j) for j, c in enumerate(codes))
            out[f"{side}_start"][i], out[f"{side}_length"][i] = at, len(codes)
            out[f"{side}_bases_lo"][i] = np.uint32(bases & 0xffffffff).astype(np.int32)
            out[f"{side}_bases_hi"][i] = np.uint32(bases >> 32).astype(np.int32)
        out["product"][i] = product
        extra[i] = (int(rs.randint(0, 24)), product, product + int(rs.randint(0, 40)))
    return out, extra


def one(n, twin):
    import ribbit_amd
    pairs, extra = random_pairs(n, 1)
    result = {"pairs": n}
    if twin:
        t0 = time.perf_counter()
        rows, pools = ribbit_amd.host_panel_pools(pairs, extra)
        result["host_twin_s"] = time.perf_counter() - t0
        result["host_twin_pools"] = pools
    with ribbit_amd.Scanner(2, 6) as sc:
        sc.panel_pools(pairs[:256], extra[:256])      # (the first call loads the code objects and sizes the buffers)
        walls = []
        for _ in range(2):
            t0 = time.perf_counter()
            rows, pools = sc.panel_pools(pairs, extra)
            walls.append(time.perf_counter() - t0)
    result.update(wall_s=walls, pools=pools, conflicts_mean=float(rows["conflicts"].mean()), dimer_mean=float(rows["dimer"].mean()))
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384,65536")
    ap.add_argument("--twin", type=int, default=4096)
    ap.add_argument("--limit", type=int, default=240, help="seconds a size may take")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=int, default=0)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.twin == args.one)
    results = []
    for n in [int(v) for v in args.sizes.split(",")]:
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n), "--twin", str(args.twin)], capture_output=True, text=True, timeout=args.limit,
                               env=dict(os.environ, RIBBIT_PROFILE="1"))
        if child.returncode != 0:
            sys.exit(f"{n} pairs: exit status {child.returncode}\n{child.stderr[-2000:]}")
        result = json.loads(child.stdout.strip().splitlines()[-1])
        stages = [m.groupdict() for m in re.finditer(r"\[panel\] pairs (?P<pairs>\d+) matrix_ms (?P<matrix_ms>[\d.]+) order_ms (?P<order_ms>[\d.]+) first_fit_ms (?P<first_fit_ms>[\d.]+)",
                                                     child.stderr) if int(m.group("pairs")) == n]
        result["device_stages_ms"] = [{k: float(v) for k, v in s.items() if k != "pairs"} for s in stages]
        results.append(result)
        print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "ribbit_hip_panel_pools on random admissible pairs (tools/panel_timing.py), MI355X", "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
