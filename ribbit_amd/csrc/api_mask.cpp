// api_mask.cpp -- the repeat-masked FASTA body of a record (mask.hip); see api_internal.h for the map of the files behind
// include/ribbit_hip.h.  The GPU form reads the bases where the load left them (dev_ascii_src) and runs on the handle's
// stream; the host twin and the BED row parser need no GPU.  stage_down, the way down of the other row outputs' inputs, is
// here beside build_coverage.
#include "bed_text.h"

namespace {

// width of a line as the format kernel takes it: 1 .. length (0 and anything longer: the whole body on one line)
int64_t effective_width(int64_t length, int32_t line_width) {
    return line_width == 0 || line_width > length ? length : line_width;
}

int64_t body_length(int64_t length, int64_t width) {
    return length == 0 ? 0 : length + (length + width - 1) / width;
}

int check_mask_args(const int32_t *intervals, size_t n, int32_t mode, int32_t line_width, const void *text, const size_t *len) {
    if (mode != RIBBIT_MASK_SOFT && mode != RIBBIT_MASK_HARD) return fail(RIBBIT_E_ARG, "mask mode %d is neither RIBBIT_MASK_SOFT nor RIBBIT_MASK_HARD", (int)mode);
    if (line_width < 0) return fail(RIBBIT_E_ARG, "line width %d is negative", (int)line_width);
    if ((!intervals && n > 0) || !text || !len) return fail(RIBBIT_E_ARG, "null argument");
    if (n > ((size_t)1 << 40)) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    return RIBBIT_OK;
}

// one decimal field of a BED row; false unless it is [-]digits within int32
bool parse_int32(const char *p, const char *end, int32_t *out) {
    bool neg = false;
    if (p < end && *p == '-') { neg = true; ++p; }
    if (p == end) return false;
    int64_t v = 0;
    for (; p < end; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = v * 10 + (*p - '0');
        if (v > ((int64_t)1 << 31)) return false;
    }
    v = neg ? -v : v;
    if (v < INT32_MIN || v > INT32_MAX) return false;
    *out = (int32_t)v;
    return true;
}

int mask_record_impl(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t mode, int32_t line_width, const char **text, size_t *len) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_mask_args(intervals, n, mode, line_width, text, len))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const char kEmpty[1] = {0};
    const int64_t length = h->length;
    if (length == 0) { *text = kEmpty; *len = 0; return RIBBIT_OK; }
    if ((rc = bind_device(h))) return rc;
    const int64_t width = effective_width(length, line_width);
    const int64_t out_len = body_length(length, width);
    const int64_t nwords = length / 32 + 1;
    if ((rc = h->rows.d_work.ensure((size_t)((out_len + 15) & ~(int64_t)15), true))) return rc;
    if ((rc = h->rows.h_mask_text.ensure((size_t)out_len, true))) return rc;
    if ((rc = build_coverage(h, intervals, n))) return rc;
    rb::launch_mask_format(h->dev_ascii_src, length, h->rows.d_mask_bits.p, nwords, mode == RIBBIT_MASK_HARD, width, out_len, h->rows.d_work.p, h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->rows.h_mask_text.p, h->rows.d_work.p, (size_t)out_len, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *text = h->rows.h_mask_text.p;
    *len = (size_t)out_len;
    return RIBBIT_OK;
}

}  // namespace

// The staged copy of the last rows stays in rows.h_mask_iv: a call with the same rows (the command-line tool hands one record's rows to
// the mask, the loci and the density) finds the bitmap as it needs it, at the price of one comparison.
bool rbapi::coverage_is(const RibbitHandle *h, const int32_t *intervals, size_t n) {
    return h->rec.coverage_valid && h->rec.coverage_n == n && (n == 0 || std::memcmp(h->rows.h_mask_iv.p, intervals, 2 * n * sizeof(int32_t)) == 0);
}

int rbapi::build_coverage(RibbitHandle *h, const int32_t *intervals, size_t n) {
    if (coverage_is(h, intervals, n)) return RIBBIT_OK;
    h->rec.coverage_valid = false;
    h->rec.overlap_valid = false;      // (what api_overlap.cpp keeps belongs to the rows of the bitmap)
    int rc;
    const size_t words = (size_t)rb::coverage_words(h->length);
    if ((rc = h->rows.d_mask_bits.ensure(words))) return rc;
    HIP_TRY(hipMemsetAsync(h->rows.d_mask_bits.p, 0, words * sizeof(uint32_t), h->stream));
    if (n) {
        if ((rc = h->rows.h_mask_iv.ensure(2 * n, true))) return rc;
        if ((rc = h->rows.d_mask_iv.ensure(2 * n, true))) return rc;
        // (the staging buffer may still be the source of the last call's copy: that call ended in a synchronise)
        std::memcpy(h->rows.h_mask_iv.p, intervals, 2 * n * sizeof(int32_t));
        HIP_TRY(hipMemcpyAsync(h->rows.d_mask_iv.p, h->rows.h_mask_iv.p, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        rb::launch_mask_coverage(h->rows.d_mask_iv.p, (int64_t)n, h->length, h->rows.d_mask_bits.p, h->stream);
        HIP_TRY(hipGetLastError());
    }
    h->rec.coverage_valid = true;
    h->rec.coverage_n = n;
    return RIBBIT_OK;
}

int rbapi::stage_down(RibbitHandle *h, const StageSegment *segs, size_t n_segs, const uint8_t **at) {
    size_t bytes = 0, filled = 0;
    for (size_t i = 0; i < n_segs; ++i) bytes += round16(segs[i].bytes);
    bytes += 16;
    int rc;
    if ((rc = h->rows.h_in.ensure(bytes, true)) || (rc = h->rows.d_in.ensure(bytes, true))) return rc;
    // (the staging buffer may still be the source of the last call's copy: that call ended in a synchronise)
    uint8_t *in = h->rows.h_in.p;
    size_t to = 0;
    for (size_t i = 0; i < n_segs; ++i) {
        at[i] = h->rows.d_in.p + to;
        if (segs[i].bytes) std::memcpy(in + to, segs[i].p, segs[i].bytes);
        filled = to + segs[i].bytes;
        to += round16(segs[i].bytes);
    }
    std::memset(in + filled, 0, bytes - filled);
    HIP_TRY(hipMemcpyAsync(h->rows.d_in.p, in, bytes, hipMemcpyHostToDevice, h->stream));
    return RIBBIT_OK;
}

namespace {

int host_mask_record_impl(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t mode, int32_t line_width,
                          char **text, size_t *len) {
    int rc;
    if ((rc = check_mask_args(intervals, n, mode, line_width, text, len))) return rc;
    if (length < 0 || (!sequence && length > 0)) return fail(RIBBIT_E_ARG, "bad sequence");
    const int64_t width = std::max<int64_t>(1, effective_width(length, line_width));
    const int64_t out_len = body_length(length, width);
    // the clipped intervals sorted by start: the mask is walked as their union without a per-base array
    const std::vector<ClippedRow> iv = clipped_sorted_rows(length, intervals, n);
    // (written where it is handed out: no second copy of a whole chromosome)
    char *out = static_cast<char *>(std::malloc((size_t)out_len + 1));
    if (!out) return fail(RIBBIT_E_NOMEM, "out of host memory");
    int64_t o = 0, masked_to = 0;      // [.., masked_to): the union of the intervals that start at or before i
    size_t next = 0;
    for (int64_t i = 0; i < length; ++i) {
        for (; next < iv.size() && iv[next].s <= i; ++next) masked_to = std::max(masked_to, iv[next].e);
        const unsigned char c = (unsigned char)sequence[i];
        out[o++] = i >= masked_to ? (char)c : mode == RIBBIT_MASK_HARD ? 'N' : (c >= 'A' && c <= 'Z') ? (char)(c | 0x20) : (char)c;
        if ((i + 1) % width == 0 || i + 1 == length) out[o++] = '\n';
    }
    *text = out;
    *len = (size_t)o;
    return RIBBIT_OK;
}

int bed_intervals_impl(const char *text, size_t len, int32_t **pairs, size_t *n) {
    if (!pairs || !n || (!text && len > 0)) return fail(RIBBIT_E_ARG, "null argument");
    std::vector<std::vector<int32_t>> rows;      // per piece: start, end of its lines
    const BedRead read = bed_read(text, len, rows, [](std::vector<int32_t> &out, const BedRow &row, const char *, const char *) {
        int32_t s = 0, e = 0;
        if (!row.ok || !parse_int32(row.start.from, row.start.to, &s) || !parse_int32(row.end.from, row.end.to, &e)) return false;
        out.push_back(s);
        out.push_back(e);
        return true;
    });
    if (read.oom) return fail(RIBBIT_E_NOMEM, "out of host memory reading BED rows");
    if (read.bad) return fail(RIBBIT_E_ARG, "BED text at byte %zu is not a row of 11 tab-separated columns with integer start and end", (size_t)(read.bad - text));
    size_t total = 0;
    for (const std::vector<int32_t> &r : rows) total += r.size();
    int rc;
    if ((rc = hand_out<int32_t>(nullptr, total, false, pairs))) return rc;
    size_t at = 0;
    for (const std::vector<int32_t> &r : rows) {
        if (!r.empty()) std::memcpy(*pairs + at, r.data(), r.size() * sizeof(int32_t));
        at += r.size();
    }
    *n = total / 2;
    return RIBBIT_OK;
}

}  // namespace

extern "C" {

int ribbit_hip_mask_record(RibbitHandle *h, const int32_t *intervals, size_t n, int32_t mode, int32_t line_width,
                           const char **text, size_t *len) {
    return guarded("the mask", [&]() -> int { return mask_record_impl(h, intervals, n, mode, line_width, text, len); });
}

int ribbit_host_mask_record(const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t mode,
                            int32_t line_width, char **text, size_t *len) {
    return guarded("the mask", [&]() -> int { return host_mask_record_impl(sequence, length, intervals, n, mode, line_width, text, len); });
}

int ribbit_bed_intervals(const char *text, size_t len, int32_t **pairs, size_t *n) {
    return guarded("reading BED rows", [&]() -> int { return bed_intervals_impl(text, len, pairs, n); });
}

void ribbit_intervals_free(int32_t *pairs) { std::free(pairs); }

}  // extern "C"
