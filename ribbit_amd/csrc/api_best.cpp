// api_best.cpp -- the best non-overlapping rows of a record (best.hip); see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form stages the rows through stage_down (it reads no coverage bitmap), runs on the handle's stream
// and keeps nothing between calls; the host twin is written from the contract, one sort and two sweeps over the whole order without the
// kernels' segments; the chosen rows' text needs no GPU either.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = (size_t)INT32_MAX;      // (the indices are int32)
constexpr size_t TOTALS_INTS = sizeof(rb::BestTotals) / sizeof(int32_t);      // the result on its way up: the totals, then the chosen rows' indices
static_assert(sizeof(rb::BestTotals) == 24, "the indices follow the totals in one buffer of ints");

int check_best_args(const int32_t *intervals, size_t n, const void *rows, const size_t *n_best, const int64_t *bases) {
    if ((!intervals && n > 0) || !rows || !n_best || !bases) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    return RIBBIT_OK;
}

int record_best_impl(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t **rows, size_t *n_best, int64_t *bases) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_best_args(intervals, n, rows, n_best, bases))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const int32_t kNone[1] = {0};
    *rows = kNone;
    *n_best = 0;
    *bases = 0;
    const int64_t length = h->length;
    if (length == 0 || n == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    RibbitHandle::RowBufs &buf = h->rows;
    const rb::BestLayout at = rb::best_layout((int64_t)n, length);
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_best.ensure(TOTALS_INTS + n, true))) return rc;
    const StageSegment down{intervals, 2 * n * sizeof(int32_t)};
    const uint8_t *d_rows = nullptr;
    if ((rc = stage_down(h, &down, 1, &d_rows))) return rc;
    uint8_t *work = buf.d_work.p;
    HIP_TRY(rb::launch_best(reinterpret_cast<const int32_t *>(d_rows), (int64_t)n, length, work, buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_best.p, work + at.totals, sizeof(rb::BestTotals), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_best.p + TOTALS_INTS, work + at.selected, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    rb::BestTotals totals;
    std::memcpy(&totals, buf.h_best.p, sizeof totals);
    if (totals.rows > n || totals.selected > totals.rows || (totals.selected == 0) != (totals.rows == 0) || totals.bases > (unsigned long long)length ||
        totals.bases < totals.selected)
        return fail(RIBBIT_E_INTERNAL, "the selection's totals contradict each other");
    *rows = buf.h_best.p + TOTALS_INTS;
    *n_best = (size_t)totals.selected;
    *bases = (int64_t)totals.bases;
    return RIBBIT_OK;
}

// ---- host twin: the contract as it is written, over the whole order at once
int host_record_best_impl(int64_t length, const int32_t *intervals, size_t n, int32_t **rows, size_t *n_best, int64_t *bases) {
    int rc;
    if ((rc = check_best_args(intervals, n, rows, n_best, bases))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    using Row = ClippedRow;
    const std::vector<Row> order =
        clipped_sorted_rows(length, intervals, n, [](const Row &a, const Row &b) { return a.e != b.e ? a.e < b.e : a.s != b.s ? a.s < b.s : a.index < b.index; });
    const size_t r = order.size();
    // forward: row k (1-based) is order[k - 1]; p(k): the rows that end at or before its start
    std::vector<int64_t> dp(r + 1, 0);
    std::vector<size_t> p(r + 1, 0);
    for (size_t k = 1; k <= r; ++k) {
        const Row &row = order[k - 1];
        p[k] = (size_t)(std::upper_bound(order.begin(), order.end(), row.s, [](int64_t s, const Row &x) { return s < x.e; }) - order.begin());
        dp[k] = std::max(dp[k - 1], row.e - row.s + dp[p[k]]);
    }
    // backward: the selected rows come out by descending position
    std::vector<int32_t> chosen;
    for (size_t k = r; k > 0;) {
        const Row &row = order[k - 1];
        if (row.e - row.s + dp[p[k]] > dp[k - 1]) {
            chosen.push_back((int32_t)row.index);
            k = p[k];
        } else {
            --k;
        }
    }
    std::reverse(chosen.begin(), chosen.end());
    if ((rc = hand_out(chosen.data(), chosen.size(), false, rows))) return rc;
    *n_best = chosen.size();
    *bases = dp[r];
    return RIBBIT_OK;
}

// ---- the chosen rows as text
int bed_rows_text_impl(const char *bed, size_t bed_len, const int32_t *rows, size_t n_rows, char **text, size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || (!rows && n_rows > 0)) return fail(RIBBIT_E_ARG, "null argument");
    // the BED text's line starts are found in pieces, and the chosen lines are copied in as many pieces
    const size_t parts = n_rows ? bed_text_parts(bed_len) : 1;
    BedLines lines;
    int rc;
    if (n_rows && (rc = lines.find(bed, bed_len, parts))) return rc;
    const size_t n_lines = lines.count();
    const size_t out_parts = std::max<size_t>(1, std::min<size_t>(parts, n_rows >> 12));
    return write_pieces(out_parts, "the chosen rows", text, len, [&](size_t k, std::string &out) {
        const size_t from = n_rows * k / out_parts, to = n_rows * (k + 1) / out_parts;
        size_t room = 0;
        for (size_t i = from; i < to; ++i) {
            if (rows[i] < 0 || (size_t)rows[i] >= n_lines) return PieceRefusal{1, i};
            room += lines[(size_t)rows[i]].size() + 2;
        }
        out.reserve(room);
        for (size_t i = from; i < to; ++i) {
            put_field(out, lines[(size_t)rows[i]]);
            out += '\n';
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) { return fail(RIBBIT_E_ARG, "entry %zu: row %d is no line of the BED text (%zu lines)", b.a, (int)rows[b.a], n_lines); });
}

}  // namespace

extern "C" {

int ribbit_hip_record_best(RibbitHandle *h, const int32_t *intervals, size_t n, const int32_t **rows, size_t *n_best, int64_t *bases) {
    return guarded("the best rows", [&]() -> int { return record_best_impl(h, intervals, n, rows, n_best, bases); });
}

int ribbit_host_record_best(int64_t length, const int32_t *intervals, size_t n, int32_t **rows, size_t *n_best, int64_t *bases) {
    return guarded("the best rows", [&]() -> int { return host_record_best_impl(length, intervals, n, rows, n_best, bases); });
}

int ribbit_bed_rows_text(const char *bed_text, size_t bed_len, const int32_t *rows, size_t n_rows, char **text, size_t *len) {
    return guarded("the chosen rows' text", [&]() -> int { return bed_rows_text_impl(bed_text, bed_len, rows, n_rows, text, len); });
}

}  // extern "C"
