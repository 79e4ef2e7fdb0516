"""Regenerates tests/golden/ssw/ref_vectors.npz: the reference SSW library's record (oracle/_ref/libssw_ref.so) for every
call test_ssw.ref_align makes in tests/test_ssw.py and tests/test_ssw_gpu.py, so that those tests keep their pin to the
reference where its sources were not there to build the library.

Needs oracle/_ref/libssw_ref.so (built by oracle/Makefile from the reference sources); no GPU: the GPU tests run against a
stand-in Scanner that answers with the reference library's own results, which is enough to enumerate their calls.

    python tests/golden/make_ssw_ref_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import pytest  # noqa: E402

import ribbit_amd  # noqa: E402
import test_ssw  # noqa: E402

if not os.path.exists(test_ssw.REF_SO):
    raise SystemExit("oracle/_ref/libssw_ref.so is not built: nothing to record from")

recorded = {}
_live = test_ssw.ref_align


def recording_ref_align(query, ref, ref_len=None, mask_len=15):
    ref_len = len(ref) if ref_len is None else ref_len
    want, cigar = _live(query, ref, ref_len, mask_len)
    recorded[test_ssw.ref_key(query, ref, ref_len, mask_len)] = ([want[n] for n, _ in test_ssw.RefResult._fields_], cigar)
    return want, cigar


class StandInScanner:
    """what test_ssw_gpu's alignment tests read from a Scanner, answered with the reference library's results"""
    def __init__(self, *a, **k):
        self.record = b""

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def load_record(self, record):
        self.record = bytes(record)

    def _pairs(self, jobs, pool):
        for j in jobs:
            query = self.record[j["query_start"]:j["query_start"] + j["query_length"]]
            motif = pool[j["motif_offset"]:j["motif_offset"] + j["atomicity"]]
            yield query, motif * (int(j["ppr_length"]) // len(motif) + 2), int(j["ppr_length"])

    def ssw_passes(self, jobs, pool, mask_len=15):
        out = np.zeros(len(jobs), ribbit_amd.ENDS_DT)
        for k, (query, ref, ppr) in enumerate(self._pairs(jobs, pool)):
            if len(query) > 8192 or ppr > 16384:
                out[k]["flag"] = -1
                continue
            w, _ = recording_ref_align(query, ref, ppr, mask_len)
            if w["sw_score"] == 0:
                out[k]["ref_end"] = -1
                continue
            out[k] = (w["sw_score"], w["ref_end"], w["query_end"], w["sw_score_next_best"], w["ref_end_next_best"],
                      w["ref_begin"], w["query_begin"], 0)
        return out

    def ssw_align_jobs(self, jobs, pool, mask_len=15):
        res = []
        for query, ref, ppr in self._pairs(jobs, pool):
            w, cigar = recording_ref_align(query, ref, ppr, mask_len)
            res.append((w, cigar if w["sw_score"] else f"{len(query)}S"))
        return res, np.full(len(jobs), 2, dtype=np.int32)


class Recorder:
    def pytest_collection_modifyitems(self, items):
        import test_ssw_gpu
        test_ssw.ref_align = test_ssw_gpu.ref_align = recording_ref_align
        test_ssw_gpu.ribbit_amd = type("StandIn", (), {"Scanner": StandInScanner, "JOB_DT": ribbit_amd.JOB_DT})


def main():
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "-m", "gpu or not gpu", os.path.join(TESTS, "test_ssw.py"),
                      os.path.join(TESTS, "test_ssw_gpu.py"), "-k", "not bed and not do_not_fit"], plugins=[Recorder()])
    if rc != 0:
        raise SystemExit(f"pytest returned {rc}: nothing written")
    keys = sorted(recorded)
    cigars = [recorded[k][1].encode() for k in keys]
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in cigars])
    np.savez_compressed(os.path.join(HERE, "ssw", "ref_vectors.npz"),
                        keys=np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), 20),
                        fields=np.array([recorded[k][0] for k in keys], dtype=np.int32).reshape(len(keys), 10),
                        cigar_off=off, cigars=np.frombuffer(b"".join(cigars), dtype=np.uint8))
    print(f"{len(keys)} reference alignments, {off[-1]} CIGAR bytes -> tests/golden/ssw/ref_vectors.npz")


if __name__ == "__main__":
    main()
