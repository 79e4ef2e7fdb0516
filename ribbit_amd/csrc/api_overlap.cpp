// api_overlap.cpp -- the rows of a record against a second set of intervals, OTHER (overlap.hip); see api_internal.h for the map of
// the files behind include/ribbit_hip.h.  The GPU form reads the coverage bitmap the mask builds of the rows (build_coverage,
// api_mask.cpp), makes a second one of OTHER with the same kernel and runs on the handle's stream; the host twin sorts the clipped
// intervals and sweeps them, without a per-base array, so that it states the contract a second time instead of repeating the
// kernels; the rows' text with the two columns needs no GPU either.
#include "bed_text.h"

namespace {

constexpr size_t MAX_INTERVALS = (size_t)INT32_MAX;      // (the counts are int32)
constexpr size_t TOTALS_INTS = sizeof(RibbitOverlapTotals) / sizeof(int32_t);      // the result on its way up: the totals, then (others, bases) per row
static_assert(sizeof(RibbitOverlapTotals) == 40 && TOTALS_INTS % 2 == 0, "the per-row values follow the totals in one buffer of ints");

int check_sets(const int32_t *rows, size_t n, const int32_t *other, size_t n_other, const void *per_row, const RibbitOverlapTotals *totals) {
    if ((!rows && n > 0) || (!other && n_other > 0) || !per_row || !totals) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_INTERVALS) return fail(RIBBIT_E_ARG, "%zu rows", n);
    if (n_other > MAX_INTERVALS) return fail(RIBBIT_E_ARG, "%zu intervals", n_other);
    return RIBBIT_OK;
}

int record_overlap_impl(RibbitHandle *h, const int32_t *rows, size_t n, const int32_t *other, size_t n_other, const int32_t **per_row,
                        RibbitOverlapTotals *totals) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_sets(rows, n, other, n_other, per_row, totals))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.h_overlap.ensure(TOTALS_INTS + 2 * n, true))) return rc;
    *per_row = buf.h_overlap.p + TOTALS_INTS;
    const int64_t length = h->length;
    if (length == 0) {
        std::memset(buf.h_overlap.p, 0, (TOTALS_INTS + 2 * n) * sizeof(int32_t));
        *totals = RibbitOverlapTotals{};
        return RIBBIT_OK;
    }
    // The staged copy of the last OTHER stays in h_overlap_iv, as the rows' does in h_mask_iv: the command-line tool asks twice
    // for one record when it writes both of its overlap outputs, and the second call finds the result where the first left it
    const bool same = h->rec.overlap_valid && coverage_is(h, rows, n) && h->rec.overlap_n == n_other &&
                      (n_other == 0 || std::memcmp(buf.h_overlap_iv.p, other, 2 * n_other * sizeof(int32_t)) == 0);
    if (!same) {
        h->rec.overlap_valid = false;
        if ((rc = bind_device(h))) return rc;
        if ((rc = build_coverage(h, rows, n))) return rc;
        const rb::OverlapLayout at = rb::overlap_layout((int64_t)n, (int64_t)n_other, length);
        if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
        uint8_t *work = buf.d_work.p;
        if (n_other) {
            if ((rc = buf.h_overlap_iv.ensure(2 * n_other, true))) return rc;
            // (the staging buffer may still be the source of the last call's copy: that call ended in a synchronise)
            std::memcpy(buf.h_overlap_iv.p, other, 2 * n_other * sizeof(int32_t));
        }
        HIP_TRY(rb::launch_overlap(buf.d_mask_bits.p, length, buf.d_mask_iv.p, (int64_t)n, buf.h_overlap_iv.p, (int64_t)n_other, work, buf.d_work.cap, at, h->stream));
        HIP_TRY(hipMemcpyAsync(buf.h_overlap.p, work + at.totals, sizeof(RibbitOverlapTotals), hipMemcpyDeviceToHost, h->stream));
        if (n) HIP_TRY(hipMemcpyAsync(buf.h_overlap.p + TOTALS_INTS, work + at.per_row, 2 * n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->rec.overlap_n = n_other;
        h->rec.overlap_valid = true;
    }
    std::memcpy(totals, buf.h_overlap.p, sizeof *totals);
    if ((size_t)totals->rows > n || (size_t)totals->other > n_other || totals->rows_hit > totals->rows || totals->other_hit > totals->other ||
        totals->both_bases > std::min(totals->rows_bases, totals->other_bases) || std::max(totals->rows_bases, totals->other_bases) > length)
        return fail(RIBBIT_E_INTERNAL, "the overlap's totals contradict each other");
    return RIBBIT_OK;
}

// ---- host twin: both sets clipped and sorted by start (clipped_sorted_rows), each merged into its runs of covered positions (CoveredRuns)
int host_record_overlap_impl(int64_t length, const int32_t *rows, size_t n, const int32_t *other, size_t n_other, int32_t **per_row,
                             RibbitOverlapTotals *totals) {
    int rc;
    if ((rc = check_sets(rows, n, other, n_other, per_row, totals))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    const std::vector<ClippedRow> a = clipped_sorted_rows(length, rows, n), b = clipped_sorted_rows(length, other, n_other);
    const CoveredRuns runs_a(a), runs_b(b);
    int32_t *out = static_cast<int32_t *>(std::calloc(std::max<size_t>(2 * n, 1), sizeof(int32_t)));
    if (!out) return fail(RIBBIT_E_NOMEM, "out of host memory for %zu rows", n);
    RibbitOverlapTotals t{};
    t.rows = (int32_t)a.size();
    t.other = (int32_t)b.size();
    t.rows_bases = runs_a.covered;
    t.other_bases = runs_b.covered;
    for (size_t i = 0, j = 0; i < runs_a.start.size() && j < runs_b.start.size();) {      // the two lists of runs side by side
        t.both_bases += std::max<int64_t>(0, std::min(runs_a.end[i], runs_b.end[j]) - std::max(runs_a.start[i], runs_b.start[j]));
        if (runs_a.end[i] < runs_b.end[j]) ++i; else ++j;
    }
    for (const ClippedRow &r : b) t.other_hit += runs_a.covered_in(r) > 0;
    // others: the rows by ascending start against OTHER by ascending start and, a second time, by ascending end: the intervals that
    // start before a row's end, less those that have ended at or before its start
    std::vector<int64_t> b_end;
    b_end.reserve(b.size());
    for (const ClippedRow &r : b) b_end.push_back(r.e);
    std::sort(b_end.begin(), b_end.end());
    size_t ended = 0;
    for (const ClippedRow &r : a) {
        while (ended < b_end.size() && b_end[ended] <= r.s) ++ended;
        const size_t started = (size_t)(std::lower_bound(b.begin(), b.end(), r.e, [](const ClippedRow &x, int64_t e) { return x.s < e; }) - b.begin());
        const int64_t bases = runs_b.covered_in(r);
        out[2 * r.index] = (int32_t)(started - ended);
        out[2 * r.index + 1] = (int32_t)bases;
        t.rows_hit += bases > 0;
    }
    *per_row = out;
    *totals = t;
    return RIBBIT_OK;
}

// ---- the rows' text with the two columns
int bed_overlap_text_impl(const char *bed, size_t bed_len, const int32_t *per_row, size_t n, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!per_row && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    // piece k writes lines [n k / parts, n (k + 1) / parts) where they belong: every line grows by two tabs and two numbers
    return write_pieces(parts, "the rows' overlap", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve(lines.start[to] - lines.start[from] + 24 * (to - from));
        for (size_t i = from; i < to; ++i) {
            put_field(out, lines[i]);
            for (const int32_t v : {per_row[2 * i], per_row[2 * i + 1]}) {
                out += '\t';
                put_number(out, v);
            }
            out += '\n';
        }
    });
}

}  // namespace

extern "C" {

int ribbit_hip_record_overlap(RibbitHandle *h, const int32_t *rows, size_t n, const int32_t *other, size_t n_other, const int32_t **per_row,
                              RibbitOverlapTotals *totals) {
    return guarded("the overlap", [&]() -> int { return record_overlap_impl(h, rows, n, other, n_other, per_row, totals); });
}

int ribbit_host_record_overlap(int64_t length, const int32_t *rows, size_t n, const int32_t *other, size_t n_other, int32_t **per_row,
                               RibbitOverlapTotals *totals) {
    return guarded("the overlap", [&]() -> int { return host_record_overlap_impl(length, rows, n, other, n_other, per_row, totals); });
}

int ribbit_bed_overlap_text(const char *bed_text, size_t bed_len, const int32_t *per_row, size_t n, char **text, size_t *len) {
    return guarded("the rows' overlap as text", [&]() -> int { return bed_overlap_text_impl(bed_text, bed_len, per_row, n, text, len); });
}

}  // extern "C"
