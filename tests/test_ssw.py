"""The product's own striped Smith-Waterman (ribbit_amd/csrc/ssw_exact.cpp) against the REFERENCE
library itself: oracle/_ref/libssw_ref.so is compiled from the reference's vendored ssw.c / ssw_cpp.cpp
(the only reference code that builds without Boost) and driven through its public Aligner API by
oracle/ssw_ref_shim.cpp.  This row (f1, alignment) is therefore pinned to real reference outputs.  Where the reference
sources were not there to build that library, the same outputs come from tests/golden/ssw/ref_vectors.npz: every call
these tests and tests/test_ssw_gpu.py make, recorded from the library by tests/golden/make_ssw_ref_vectors.py."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import ribbit_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libssw_ref.so")
REF_VECTORS = os.path.join(ROOT, "tests", "golden", "ssw", "ref_vectors.npz")


class RefResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sw_score", "sw_score_next_best", "ref_begin", "ref_end", "query_begin", "query_end",
                                         "ref_end_next_best", "mismatches", "flag", "cigar_len")]


_ref = None
_stored = None


def ref_key(query: bytes, ref: bytes, ref_len: int, mask_len: int) -> bytes:
    return hashlib.sha1(b"%d|%d|%d|" % (len(query), ref_len, mask_len) + query + b"|" + ref).digest()


def _stored_align(query: bytes, ref: bytes, ref_len: int, mask_len: int):
    """the reference library's record for this call from tests/golden/ssw/ref_vectors.npz"""
    global _stored
    if _stored is None:
        z = np.load(REF_VECTORS)
        _stored = ({k.tobytes(): i for i, k in enumerate(z["keys"])}, z["fields"], z["cigar_off"], z["cigars"].tobytes())
    index, fields, off, text = _stored
    i = index.get(ref_key(query, ref, ref_len, mask_len))
    assert i is not None, ("no stored reference alignment for this call: regenerate tests/golden/ssw/ref_vectors.npz "
                           "with tests/golden/make_ssw_ref_vectors.py", query[:60], ref_len, mask_len)
    return {n: int(v) for (n, _), v in zip(RefResult._fields_, fields[i])}, text[off[i]:off[i + 1]].decode()


def ref_align(query: bytes, ref: bytes, ref_len=None, mask_len=15):
    global _ref
    ref_len = len(ref) if ref_len is None else ref_len
    if _ref is None:
        if not os.path.exists(REF_SO):
            return _stored_align(query, ref, ref_len, mask_len)
        _ref = C.CDLL(REF_SO)
        _ref.ref_ssw_align.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(RefResult), C.c_char_p, C.c_int]
    out = RefResult()
    cap = 16 * (len(query) + len(ref)) + 64
    buf = C.create_string_buffer(cap)
    _ref.ref_ssw_align(query, ref, ref_len, mask_len, C.byref(out), buf, cap)
    return {n: getattr(out, n) for n, _ in RefResult._fields_}, buf.value.decode()


def _check(query, ref, ref_len=None):
    want, wc = ref_align(query, ref, ref_len)
    got, gc = ribbit_amd.ssw_align(query, ref, ref_len)
    assert gc == wc, (query, ref, ref_len, gc, wc)
    assert got == want, (query, ref, ref_len, got, want)


def _rand(rs, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rs.randint(0, len(alphabet), size=n)])


def _mutate(rs, s: bytes, rate: float) -> bytes:
    out = bytearray()
    for c in s:
        r = rs.random_sample()
        if r < rate * 0.8:
            out.append(rs.choice([x for x in b"ACGT" if x != c]))
        elif r < rate * 0.9:
            out.append(c); out.append(b"ACGT"[rs.randint(0, 4)])
        elif r < rate:
            pass
        else:
            out.append(c)
    return bytes(out)


def test_simple_cases():
    _check(b"ACGTACGTACGT", b"ACGTACGTACGTACGT")
    _check(b"AAAAAAAAAA", b"AAAAAAAAAAAAAAA")
    _check(b"ACGT", b"TTTTACGTTTTT")
    _check(b"ACGTTTACGT", b"ACGTACGT" * 3)
    _check(b"GATTACA", b"GATTTACAGATTACA")
    _check(b"CAGCAGCAGCTGCAGCAG", b"CAG" * 9)


@pytest.mark.parametrize("seed", range(12))
def test_repeat_like_jobs_match_reference(seed):
    # the shape ribbit produces: query = an impure tandem repeat, reference = the pure motif repeated past ppr_length
    rs = np.random.RandomState(100 + seed)
    for _ in range(120):
        m = int(rs.randint(1, 30))
        motif = _rand(rs, m)
        units = int(rs.randint(2, 40))
        rot = int(rs.randint(0, m))
        pure = (motif * (units + 2))[rot:rot + m * units + int(rs.randint(0, m))]
        query = _mutate(rs, pure, float(rs.choice([0.0, 0.03, 0.1, 0.2])))
        if not query:
            continue
        ppr_len = len(query) + m + int(0.15 * len(query))
        ref = motif * (ppr_len // m + 2)
        _check(query, ref, ppr_len)


@pytest.mark.parametrize("seed", range(8))
def test_the_periodic_finish_equals_the_alignment_on_the_spelt_out_reference(seed):
    """Refinement finishes an alignment whose end points and path come from the GPU without its reference string: the
    reference base at position j is motif[j % atom] (ssw_finish_with_path_periodic).  Host twin of that route (passes, path as
    run-length operations, periodic finish) against ribbit_ssw_align -- which the tests above pin to the reference library -- on
    the spelt-out string: every field and the CIGAR, for the shape ribbit produces and for queries unrelated to the motif,
    with unknown bases, lower case, motifs of one base and queries shorter than the motif."""
    rs = np.random.RandomState(4100 + seed)
    for k in range(150):
        m = int(rs.randint(1, 40))
        motif = _rand(rs, m, b"ACGTN" if rs.random_sample() < 0.1 else b"ACGT")
        if k % 3 == 2:
            query = _rand(rs, int(rs.randint(1, 200)), b"ACGTNacgt" if rs.random_sample() < 0.3 else b"ACGT")
        else:
            units = int(rs.randint(1, 40))
            rot = int(rs.randint(0, m))
            pure = (motif * (units + 2))[rot:rot + m * units + int(rs.randint(0, m))]
            query = _mutate(rs, pure, float(rs.choice([0.0, 0.03, 0.1, 0.25])))
        if not query:
            continue
        ppr_len = len(query) + m + int(0.15 * len(query))
        ref = motif * (ppr_len // m + 2)
        want, want_cigar = ribbit_amd.ssw_align(query, ref, ppr_len)
        got, got_cigar = ribbit_amd.ssw_align_periodic(query, motif, ppr_len)
        assert got_cigar == want_cigar and got == want, (query, motif, ppr_len, got, got_cigar, want, want_cigar)


@pytest.mark.parametrize("seed", range(6))
def test_random_pairs_match_reference(seed):
    rs = np.random.RandomState(500 + seed)
    for _ in range(150):
        q = _rand(rs, int(rs.randint(1, 120)), b"ACGTN" if rs.random_sample() < 0.2 else b"ACGT")
        r = _rand(rs, int(rs.randint(1, 200)))
        _check(q, r)


def test_long_alignments_take_the_16bit_path():
    rs = np.random.RandomState(7)
    for n in (130, 200, 600, 2500):
        motif = _rand(rs, int(rs.randint(2, 12)))
        pure = (motif * (n // len(motif) + 2))[:n]
        query = _mutate(rs, pure, 0.05)
        ppr_len = len(query) + len(motif) + int(0.15 * len(query))
        _check(query, motif * (ppr_len // len(motif) + 2), ppr_len)      # scores > 255
    q = _rand(rs, 3000)
    _check(q, _mutate(rs, q, 0.1))


def test_lowercase_and_unknown_bases():
    _check(b"acgtacgtnnacgt", b"ACGTACGTACGTACGT")
    _check(b"ACGTRYACGT", b"ACGTACGTACGT")


@pytest.mark.parametrize("seed", range(3))
def test_long_pairs_match_reference(seed):
    """long alignments (the 16-bit pass after the byte pass overflows): repeats of 130..3000 bases at mutation rates up to 45 %,
    indel-rich ones, unknown bases, references shorter and longer than the query, and scores just above the 255 threshold.
    (Round 2 tried this pass on 16 lanes where the library has 8, on the argument that the striped recurrence computes the
    exact matrix whatever the lane count.  It does not in every cell: `ref_end_next_best` came out 959 for the library's 970
    on a case of test_repeat_like_jobs_match_reference, so the lane count is part of the result and stays the library's.)"""
    rs = np.random.RandomState(5200 + seed)
    for _ in range(70):
        n = int(rs.choice([130, 160, 200, 255, 256, 257, 300, 400, 513, 700, 1000, 1500, 2200, 3000]))
        motif = _rand(rs, int(rs.randint(1, 60)))
        pure = (motif * (n // len(motif) + 2))[:n]
        q = _mutate(rs, pure, float(rs.choice([0.0, 0.03, 0.1, 0.25, 0.45])))
        if rs.random_sample() < 0.25:                      # a long deletion or a foreign insert moves the path off the diagonal
            cut = int(rs.randint(5, 80))
            q = q[:len(q) // 2] + q[len(q) // 2 + cut:] if rs.random_sample() < 0.5 else q[:len(q) // 3] + _rand(rs, cut) + q[len(q) // 3:]
        if rs.random_sample() < 0.15:
            q = bytes(b"N"[0] if rs.random_sample() < 0.03 else c for c in q)
        ref_len = int(rs.choice([len(q) // 2 + 1, len(q) + len(motif) + int(0.15 * len(q)), 2 * len(q)]))
        ref = motif * (ref_len // len(motif) + 2)
        _check(q, ref, ref_len)
    for _ in range(40):                                    # just over the threshold: 127..140 matching bases in unrelated flanks
        core = _rand(rs, int(rs.randint(127, 141)))
        q = _rand(rs, int(rs.randint(0, 60))) + core + _rand(rs, int(rs.randint(0, 60)))
        ref = _rand(rs, int(rs.randint(0, 80))) + core + _rand(rs, int(rs.randint(0, 80)))
        _check(q, ref)


def test_alignment_longer_than_the_distance_filter_gets_no_cigar():
    """Filter().distance_filter = 32767 (ssw_cpp.h:58-63, ssw.c:893-896): an alignment that spans more reference or query
    than that keeps its scores and end points but no path is searched.  With match +2 the 16-bit score saturates after
    16384 matching bases, long before that span, so the filter is only reachable by a very impure repeat: 31 % substitutions
    keep the score of a 36-kb alignment under 32767.  The product returns the reference library's record either way, and a
    pure repeat of the same length shows the saturation instead (16384 matches, the rest soft-clipped)"""
    rs = np.random.RandomState(12)
    motif = _rand(rs, 7)
    n = 36_000
    pure = bytearray((motif * (n // len(motif) + 2))[:n])
    impure = bytearray(pure)
    for i in np.nonzero(rs.random_sample(n) < 0.31)[0]:
        impure[i] = int(rs.choice([c for c in b"ACGT" if c != impure[i]]))
    ref_len = n + 2000
    ref = motif * (ref_len // len(motif) + 2)
    spans = []
    for q in (bytes(impure), bytes(pure)):
        want, wc = ref_align(q, ref, ref_len)
        got, gc = ribbit_amd.ssw_align(q, ref, ref_len)
        assert (got, gc) == (want, wc)
        spans.append((want["query_end"] - want["query_begin"], want["sw_score"], wc))
    # filtered: the span exceeds the limit, the score does not saturate, and the CIGAR holds no aligned operation at all
    # (the wrapper still writes the leading soft clip)
    assert spans[0][0] > 32767 and spans[0][1] < 32767 and not any(c in spans[0][2] for c in "=XID")
    # saturated: the score stops at 32767 after 16384 matches, the rest of the query is clipped
    assert spans[1][1] == 32767 and spans[1][0] == 16383 and spans[1][2].startswith("16384=")
