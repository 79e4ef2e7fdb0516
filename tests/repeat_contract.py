"""The repeat-FASTA contract stated with numpy (tests/test_repeat_fasta.py, tests/test_repeat_fasta_gpu.py): one entry per
(start, end) pair, in order, with every bound clipped to the record in 64-bit arithmetic."""
import numpy as np


def repeat_entries(name, seq: bytes, intervals, flank: int = 100) -> bytes:
    name = name.encode() if isinstance(name, str) else bytes(name)
    L, F = len(seq), int(flank)
    out = []
    for s, e in np.asarray(intervals, dtype=np.int64).reshape(-1, 2).tolist():
        s = min(max(s, 0), L)
        e = min(max(e, s), L)
        lo, hi = max(s - F, 0), min(e + F, L)
        out.append(b">%s:%d-%d flank=%d,%d\n%s\n" % (name, s, e, s - lo, hi - e, seq[lo:hi]))
    return b"".join(out)


def repeat_fasta(records, beds, flank: int = 100) -> bytes:
    """records: [(name as the reader hands it out, bases)]; beds: the BED text of each record"""
    import ribbit_amd
    return b"".join(repeat_entries(name, seq, ribbit_amd.bed_intervals(bed), flank) for (name, seq), bed in zip(records, beds))
