"""The masked-FASTA contract stated with numpy (tests/test_mask.py, tests/test_mask_gpu.py): the union of the clipped
half-open rows, then the mode's byte rule, then lines of `width` bytes each ending in a newline (0: one line)."""
import numpy as np


def masked_body(seq: bytes, intervals, mode: str = "soft", width: int = 60) -> bytes:
    L = len(seq)
    cov = np.zeros(L, bool)
    for s, e in np.asarray(intervals, dtype=np.int64).reshape(-1, 2):
        s, e = max(int(s), 0), min(int(e), L)
        if s < e:
            cov[s:e] = True
    b = np.frombuffer(seq, np.uint8).copy()
    if mode == "soft":
        upper = (b >= ord("A")) & (b <= ord("Z"))
        b[cov & upper] |= 0x20
    else:
        b[cov] = ord("N")
    body = b.tobytes()
    if L == 0:
        return b""
    w = L if width == 0 else width
    return b"".join(body[i:i + w] + b"\n" for i in range(0, L, w))


def masked_fasta(records, beds, mode: str = "soft", width: int = 60) -> bytes:
    """records: [(name as the reader hands it out, bases)]; beds: the BED text of each record"""
    import ribbit_amd
    return b"".join(b">" + name.encode() + b"\n" + masked_body(seq, ribbit_amd.bed_intervals(bed), mode, width)
                    for (name, seq), bed in zip(records, beds))
