"""The contract of the merged loci and the density track stated with numpy (tests/test_loci.py, tests/test_loci_gpu.py):
a per-base coverage array of the clipped half-open rows, its runs, the runs joined over gaps of at most `gap`, then every
non-empty row counted into the locus that holds its start; and the coverage summed per window."""
import numpy as np

LOCUS_FIELDS = ("start", "end", "rows", "covered", "best_row")


def _clipped(length, intervals):
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    return np.maximum(iv[:, 0], 0), np.minimum(iv[:, 1], length)


def coverage(length, intervals):
    cov = np.zeros(length, bool)
    for s, e in zip(*_clipped(length, intervals)):
        if s < e:
            cov[s:e] = True
    return cov


def record_loci(length, intervals, gap=0):
    """-> list of (start, end, rows, covered, best_row), by ascending start"""
    cov = coverage(length, intervals)
    edge = np.diff(np.concatenate([[0], cov.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
    loci = []          # [start, end, covered]
    for s, e in zip(starts.tolist(), ends.tolist()):
        if loci and s - loci[-1][1] <= gap:
            loci[-1][1] = e
            loci[-1][2] += e - s
        else:
            loci.append([s, e, e - s])
    rows = [0] * len(loci)
    best = [(-1, 0)] * len(loci)      # (length, -index): the largest wins
    lstart = np.array([l[0] for l in loci], np.int64)
    for i, (s, e) in enumerate(zip(*_clipped(length, intervals))):
        if s >= e:
            continue
        k = int(np.searchsorted(lstart, s, side="right")) - 1
        assert k >= 0 and loci[k][0] <= s and e <= loci[k][1]      # every non-empty row lies in exactly one locus
        rows[k] += 1
        best[k] = max(best[k], (int(e - s), -i))
    return [(l[0], l[1], rows[k], l[2], -best[k][1]) for k, l in enumerate(loci)]


def record_density(length, intervals, window):
    cov = coverage(length, intervals)
    n = -(-length // window)
    upto = np.concatenate([[0], np.cumsum(cov, dtype=np.int64)])          # covered positions before p
    edges = np.minimum(np.arange(n + 1, dtype=np.int64) * window, length)
    return (upto[edges[1:]] - upto[edges[:-1]]).tolist()


def loci_lines(name, bed, loci):
    """the loci file's lines for one record, in plain Python: name, the locus's first four values, then the last ten columns
    of its best row (bed: the record's BED text; loci: tuples as record_loci returns them)"""
    rows = bed.splitlines()
    out = []
    for start, end, nrows, covered, best in loci:
        out.append("\t".join([name, str(start), str(end), str(nrows), str(covered)] + rows[best].split("\t")[-10:]) + "\n")
    return "".join(out)


def density_lines(name, length, window, density):
    return "".join(f"{name}\t{k * window}\t{min((k + 1) * window, length)}\t{v}\n" for k, v in enumerate(density))
