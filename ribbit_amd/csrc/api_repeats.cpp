// api_repeats.cpp -- every row's bases with their flanks as FASTA entries (repeats.hip); see api_internal.h for the map of the
// files behind include/ribbit_hip.h.  The GPU form reads the bases where the load left them (dev_ascii_src), runs on the handle's
// stream and hands the text back in batches of at most the handle's text budget; the host twin writes the whole text at once.
#include "bed_text.h"

namespace {

constexpr size_t REPEAT_TEXT_BUDGET = (size_t)64 << 20;
constexpr size_t MAX_NAME = (size_t)1 << 24;     // (a record name is a FASTA header line up to its first space)

int check_repeat_args(const char *name, const int32_t *intervals, size_t n, int32_t flank, const void *text, const size_t *len) {
    if (flank < 0) return fail(RIBBIT_E_ARG, "flank %d is negative", (int)flank);
    if (!name || (!intervals && n > 0) || !text || !len) return fail(RIBBIT_E_ARG, "null argument");
    if (n > ((size_t)1 << 40)) return fail(RIBBIT_E_ARG, "%zu intervals", n);
    if (std::strlen(name) > MAX_NAME) return fail(RIBBIT_E_ARG, "a name of %zu bytes", std::strlen(name));
    return RIBBIT_OK;
}

int repeat_sequences_impl(RibbitHandle *h, const char *name, const int32_t *intervals, size_t n, int32_t flank, const char **text,
                          size_t *len, size_t *rows_done) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_repeat_args(name, intervals, n, flank, text, len))) return rc;
    if (!rows_done) return fail(RIBBIT_E_ARG, "null argument");
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const char kEmpty[1] = {0};
    if (n == 0) { *text = kEmpty; *len = 0; *rows_done = 0; return RIBBIT_OK; }
    if ((rc = bind_device(h))) return rc;
    const int64_t length = h->length;
    const size_t name_len = std::strlen(name);
    const size_t budget = std::min(h->rows.rep_budget ? h->rows.rep_budget : REPEAT_TEXT_BUDGET, (size_t)1 << 50);
    // Every entry is at least 17 + name_len + min(F, L) bytes (its body holds a flank or reaches both ends of the record), so
    // no more rows than m can fit the budget: only those go up and through the scan, however many rows are left.
    const size_t min_entry = 17 + name_len + (size_t)std::min<int64_t>(flank, length);
    const size_t m = std::min(n, budget / min_entry + 1);
    const size_t name_words = (name_len + 4) / 4;        // the name follows the rows in the same buffer
    if ((rc = h->rows.h_rep_iv.ensure(2 * m + name_words, true))) return rc;
    if ((rc = h->rows.d_rep_iv.ensure(2 * m + name_words, true))) return rc;
    if ((rc = h->rows.d_rep_off.ensure(m + 1, true))) return rc;
    const size_t scratch = rb::repeat_scan_scratch_bytes((int64_t)m);
    if ((rc = h->rows.d_work.ensure(scratch, true))) return rc;
    if ((rc = h->rows.d_rep_pick.ensure(2))) return rc;
    if ((rc = h->rows.h_rep_pick.ensure(2))) return rc;
    // (the staging buffers may still be the source or target of the last call's copies: that call ended in a synchronise)
    std::memcpy(h->rows.h_rep_iv.p, intervals, 2 * m * sizeof(int32_t));
    std::memcpy(h->rows.h_rep_iv.p + 2 * m, name, name_len + 1);
    HIP_TRY(hipMemcpyAsync(h->rows.d_rep_iv.p, h->rows.h_rep_iv.p, (2 * m + name_words) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(rb::launch_repeat_offsets(h->rows.d_rep_iv.p, (int64_t)m, length, flank, (int32_t)name_len, (int64_t)budget, h->rows.d_rep_off.p,
                                      h->rows.d_rep_pick.p, h->rows.d_work.p, h->rows.d_work.cap, h->stream));
    HIP_TRY(hipMemcpyAsync(h->rows.h_rep_pick.p, h->rows.d_rep_pick.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int64_t k = h->rows.h_rep_pick.p[0], total = h->rows.h_rep_pick.p[1];
    if (k < 1 || (size_t)k > m || total <= 0) return fail(RIBBIT_E_INTERNAL, "repeat batch of %lld rows, %lld bytes", (long long)k, (long long)total);
    // the text buffers: at least twice the last size when they grow, never more than the budget unless one entry is larger
    const size_t padded = (size_t)((total + 15) & ~(int64_t)15);
    const size_t want = std::max(padded, std::min(2 * padded, (budget + 15) & ~(size_t)15));
    if (padded > h->rows.d_rep_text.cap && (rc = h->rows.d_rep_text.ensure(want))) return rc;
    if ((size_t)total > h->rows.h_rep_text.cap && (rc = h->rows.h_rep_text.ensure(want))) return rc;
    if ((rc = h->rows.d_rep_span_row.ensure((size_t)((total + rb::REPEAT_SPAN - 1) / rb::REPEAT_SPAN) + 1, true))) return rc;
    rb::launch_repeat_format(h->dev_ascii_src, length, h->rows.d_rep_iv.p, h->rows.d_rep_off.p, k, total, flank,
                             reinterpret_cast<const char *>(h->rows.d_rep_iv.p + 2 * m), (int32_t)name_len, h->rows.d_rep_span_row.p, h->rows.d_rep_text.p,
                             h->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->rows.h_rep_text.p, h->rows.d_rep_text.p, (size_t)total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *text = h->rows.h_rep_text.p;
    *len = (size_t)total;
    *rows_done = (size_t)k;
    return RIBBIT_OK;
}

// a plain loop over the rows: the reference the GPU form is tested against
int host_repeat_sequences_impl(const char *name, const char *sequence, int64_t length, const int32_t *intervals, size_t n, int32_t flank,
                               char **text, size_t *len) {
    int rc;
    if ((rc = check_repeat_args(name, intervals, n, flank, text, len))) return rc;
    if (length < 0 || (!sequence && length > 0)) return fail(RIBBIT_E_ARG, "bad sequence");
    std::string out;
    auto put = [&](int64_t v) { put_number(out, v); };
    for (size_t i = 0; i < n; ++i) {
        const int64_t s = std::min(std::max<int64_t>(intervals[2 * i], 0), length);
        const int64_t e = std::min(std::max<int64_t>(intervals[2 * i + 1], s), length);
        const int64_t lo = std::max<int64_t>(s - flank, 0), hi = std::min<int64_t>(e + flank, length);
        out += '>';
        out += name;
        out += ':';
        put(s);
        out += '-';
        put(e);
        out += " flank=";
        put(s - lo);
        out += ',';
        put(hi - e);
        out += '\n';
        out.append(sequence + lo, (size_t)(hi - lo));
        out += '\n';
    }
    if ((rc = hand_out(out.data(), out.size(), true, text))) return rc;
    *len = out.size();
    return RIBBIT_OK;
}

}  // namespace

extern "C" {

int ribbit_hip_repeat_sequences(RibbitHandle *h, const char *name, const int32_t *intervals, size_t n, int32_t flank,
                                const char **text, size_t *len, size_t *rows_done) {
    return guarded("the repeat sequences", [&]() -> int { return repeat_sequences_impl(h, name, intervals, n, flank, text, len, rows_done); });
}

int ribbit_host_repeat_sequences(const char *name, const char *sequence, int64_t length, const int32_t *intervals,
                                 size_t n, int32_t flank, char **text, size_t *len) {
    return guarded("the repeat sequences", [&]() -> int { return host_repeat_sequences_impl(name, sequence, length, intervals, n, flank, text, len); });
}

int ribbit_hip_debug_set_repeat_text_budget(RibbitHandle *h, size_t bytes) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    h->rows.rep_budget = bytes;
    return RIBBIT_OK;
}

}  // extern "C"
