// api_interruptions.cpp -- every row's CIGAR decoded into interruptions and the pure stretch (interruptions.hip); see
// api_internal.h for the map of the files behind include/ribbit_hip.h.  The GPU form stages the rows, the offsets and the CIGARs
// through stage_down, reads the bases where the load left them (dev_ascii_src), runs on the handle's stream and
// keeps nothing between calls; it synchronises twice: once for the counts (which size the observed text and carry what the
// grammar check found), once for the results.  The host twin is the contract as a plain loop over the rows and their ops, and
// words every refusal: when the GPU reports an offending byte or row, the twin's walk over the same CIGARs writes the message.
// The CIGARs of a BED text and the two outputs' texts need no GPU.
#include "bed_text.h"

namespace {

constexpr size_t MAX_ROWS = BED_MAX_ROWS;

inline bool is_match(char c) { return c == '=' || c == 'M'; }
inline bool is_op(char c) { return is_match(c) || c == 'X' || c == 'I' || c == 'D'; }

int check_interruption_args(const int32_t *intervals, const int32_t *motif_lengths, size_t n, const char *cigars, const int32_t *offsets, const void *rows,
                            const void *sites, const size_t *n_sites, const void *observed, const void *observed_offsets) {
    if (((!intervals || !motif_lengths || !offsets) && n > 0) || !rows || !sites || !n_sites || !observed || !observed_offsets) return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu rows", n);
    if (n == 0) return RIBBIT_OK;
    if (offsets[0] != 0) return fail(RIBBIT_E_ARG, "the CIGARs' offsets start at %d, not at 0", (int)offsets[0]);
    // (an int32 offset cannot reach 2^31: a pool of 2^31 bytes or more shows as offsets that do not ascend)
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i])
            return fail(RIBBIT_E_ARG, "row %zu: the CIGARs' offsets do not ascend (%d, then %d; a pool has fewer than 2^31 bytes)", i, (int)offsets[i], (int)offsets[i + 1]);
        if (motif_lengths[i] < 1) return fail(RIBBIT_E_ARG, "row %zu: a motif of %d bases", i, (int)motif_lengths[i]);
    }
    if (offsets[n] > 0 && !cigars) return fail(RIBBIT_E_ARG, "null argument");
    return RIBBIT_OK;
}

// One row's CIGAR, cigars[from .. to), walked as the contract says: on_op(kind letter, length, q before the op, offset of the op's
// first digit, offset behind its letter) for every op; then the sums are checked.  -> RIBBIT_OK with *query set, or the refusal.
template <typename OnOp>
int walk_row(size_t row, int64_t s, const char *cigars, int32_t from, int32_t to, int64_t *query, OnOp on_op) {
    int64_t q = 0, all = 0, value = 0;
    int digits = 0;
    int32_t first_digit = from;
    for (int32_t p = from; p < to; ++p) {
        const char c = cigars[p];
        if (c >= '0' && c <= '9') {
            if (digits == 0) first_digit = p;
            value = digits < 10 ? value * 10 + (c - '0') : (int64_t)INT32_MAX + 1;
            digits = std::min(digits + 1, 11);
            continue;
        }
        if (!is_op(c)) return fail(RIBBIT_E_ARG, "the CIGARs' byte %d (row %zu) is neither a digit nor one of = M X I D", (int)p, row);
        if (digits == 0) return fail(RIBBIT_E_ARG, "the CIGARs' byte %d (row %zu) is an op letter without a length before it", (int)p, row);
        if (digits > 10) return fail(RIBBIT_E_ARG, "the CIGARs' byte %d (row %zu) ends an op of more than ten digits", (int)p, row);
        if (value < 1 || value > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "the CIGARs' byte %d (row %zu) ends an op whose length is not 1 .. 2147483647", (int)p, row);
        on_op(c, value, q, first_digit, p + 1);
        all += value;
        if (c != 'D') q += value;
        value = 0;
        digits = 0;
    }
    if (digits) return fail(RIBBIT_E_ARG, "the CIGARs' byte %d (row %zu) is the row's end, behind digits without an op letter", (int)to, row);
    if (all > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "row %zu: the CIGAR's op lengths sum to %lld, more than 2147483647", row, (long long)all);
    if (s + q > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "row %zu: its start %lld and its CIGAR's query length %lld do not fit int32 together", row, (long long)s, (long long)q);
    *query = q;
    return RIBBIT_OK;
}

// the refusal of the first row that has one (what the GPU found, in the twin's words)
int first_refusal(const int32_t *intervals, size_t n, const char *cigars, const int32_t *offsets) {
    for (size_t i = 0; i < n; ++i) {
        int64_t query = 0;
        const int rc = walk_row(i, intervals[2 * i], cigars, offsets[i], offsets[i + 1], &query, [](char, int64_t, int64_t, int32_t, int32_t) {});
        if (rc) return rc;
    }
    return RIBBIT_OK;
}

int record_interruptions_impl(RibbitHandle *h, const int32_t *intervals, const int32_t *motif_lengths, size_t n, const char *cigars, const int32_t *offsets,
                              const RibbitRowPurity **rows, const RibbitInterruption **sites, size_t *n_sites, const char **observed, const int32_t **observed_offsets) {
    if (!h) return fail(RIBBIT_E_ARG, "null handle");
    int rc;
    if ((rc = check_interruption_args(intervals, motif_lengths, n, cigars, offsets, rows, sites, n_sites, observed, observed_offsets))) return rc;
    if (!h->loaded) return fail(RIBBIT_E_STATE, "no record loaded");
    static const RibbitRowPurity kNoRows[1] = {};
    static const RibbitInterruption kNoSites[1] = {};
    static const char kNoText[1] = {0};
    static const int32_t kNoOffsets[1] = {0};
    *rows = kNoRows;
    *sites = kNoSites;
    *n_sites = 0;
    *observed = kNoText;
    *observed_offsets = kNoOffsets;
    if (n == 0) return RIBBIT_OK;
    if ((rc = bind_device(h))) return rc;
    // down: the rows | the offsets | the CIGARs, each on a 16-byte boundary, the CIGARs zero-filled to one 16 bytes behind theirs
    const size_t pool = (size_t)offsets[n];
    const rb::InterruptionLayout at = rb::interruptions_layout((int64_t)n, pool);
    RibbitHandle::RowBufs &buf = h->rows;
    if ((rc = buf.d_work.ensure(at.bytes, true))) return rc;
    if ((rc = buf.h_int_totals.ensure(sizeof(rb::InterruptionTotals)))) return rc;
    const StageSegment down[3] = {{intervals, 2 * n * sizeof(int32_t)}, {offsets, (n + 1) * sizeof(int32_t)}, {cigars, pool}};
    const uint8_t *d_in[3];
    if ((rc = stage_down(h, down, 3, d_in))) return rc;
    uint8_t *work = buf.d_work.p;
    HIP_TRY(rb::launch_interruptions(reinterpret_cast<const int32_t *>(d_in[0]), reinterpret_cast<const int32_t *>(d_in[1]), d_in[2], (int64_t)n, pool, h->length,
                                     work, buf.d_work.cap, at, h->stream));
    HIP_TRY(hipMemcpyAsync(buf.h_int_totals.p, work + at.totals, sizeof(rb::InterruptionTotals), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    rb::InterruptionTotals totals;
    std::memcpy(&totals, buf.h_int_totals.p, sizeof totals);
    if (totals.bad_at != 0xffffffffu || totals.bad_row != 0xffffffffu) {
        if ((rc = first_refusal(intervals, n, cigars, offsets))) return rc;
        return fail(RIBBIT_E_INTERNAL, "the GPU refused the CIGARs (byte %u, row %u) and the host does not", totals.bad_at, totals.bad_row);
    }
    if (totals.sites > totals.runs || totals.runs > totals.ops || totals.ops > rb::interruptions_op_cap(pool) - 1)
        return fail(RIBBIT_E_INTERNAL, "the interruptions' counts contradict each other (%u ops, %u runs, %u interruptions)", totals.ops, totals.runs, totals.sites);
    if (totals.observed > (unsigned long long)INT32_MAX)
        return fail(RIBBIT_E_ARG, "the interruptions' observed bases are more than 2147483647 bytes");
    if (totals.observed > 0 && !h->dev_ascii_src) return fail(RIBBIT_E_STATE, "the record's bases are not resident on the device");
    // up: the rows | the interruptions | their offsets into the observed bases | those bases
    const size_t m = totals.sites, text = (size_t)totals.observed;
    const size_t out_sites = n * sizeof(RibbitRowPurity), out_off = out_sites + m * sizeof(RibbitInterruption), out_text = out_off + round16((m + 1) * sizeof(int32_t)),
                 out_bytes = out_text + round16(text) + 16;
    if ((rc = buf.h_int.ensure(out_bytes, true))) return rc;
    uint8_t *up = buf.h_int.p;
    if (text) {
        if ((rc = buf.d_int_text.ensure(round16(text) + 16, true))) return rc;
        HIP_TRY(rb::launch_interruption_gather(h->dev_ascii_src, work, at, totals.sites, (int64_t)text, buf.d_int_text.p, h->stream));
        HIP_TRY(hipMemcpyAsync(up + out_text, buf.d_int_text.p, text, hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipMemcpyAsync(up, work + at.rows, n * sizeof(RibbitRowPurity), hipMemcpyDeviceToHost, h->stream));
    if (m) HIP_TRY(hipMemcpyAsync(up + out_sites, work + at.sites, m * sizeof(RibbitInterruption), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(up + out_off, work + at.offsets32, (m + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    up[out_text + text] = 0;
    *rows = reinterpret_cast<const RibbitRowPurity *>(up);
    *sites = reinterpret_cast<const RibbitInterruption *>(up + out_sites);
    *n_sites = m;
    *observed = reinterpret_cast<const char *>(up + out_text);
    *observed_offsets = reinterpret_cast<const int32_t *>(up + out_off);
    return RIBBIT_OK;
}

// ---- host twin: the contract as it is written
int host_record_interruptions_impl(const char *sequence, int64_t length, const int32_t *intervals, const int32_t *motif_lengths, size_t n, const char *cigars,
                                   const int32_t *offsets, RibbitRowPurity **rows, RibbitInterruption **sites, size_t *n_sites, char **observed,
                                   int32_t **observed_offsets) {
    int rc;
    if ((rc = check_interruption_args(intervals, motif_lengths, n, cigars, offsets, rows, sites, n_sites, observed, observed_offsets))) return rc;
    if (length < 0 || length > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "a record of %lld bases", (long long)length);
    if (!sequence && length > 0) return fail(RIBBIT_E_ARG, "null argument");
    std::vector<RibbitRowPurity> per_row(n);
    std::vector<RibbitInterruption> found;
    std::vector<int32_t> text_at{0};
    std::string text;
    struct Site { int64_t start, end, x, ins, del; int32_t at, behind; };      // (64-bit until the row's sums have been checked)
    std::vector<Site> of_row;
    for (size_t i = 0; i < n; ++i) {
        const int64_t s = intervals[2 * i];
        of_row.clear();
        bool in_stretch = false, in_site = false;
        int64_t stretch_from = 0, stretch_to = 0, best = 0, pure_from = 0, pure_to = 0, query = 0;
        auto close_stretch = [&]() {
            if (in_stretch && stretch_to - stretch_from > best) {      // (a later stretch of the same length does not replace it: the leftmost)
                best = stretch_to - stretch_from;
                pure_from = stretch_from;
                pure_to = stretch_to;
            }
            in_stretch = false;
        };
        if ((rc = walk_row(i, s, cigars, offsets[i], offsets[i + 1], &query, [&](char c, int64_t len, int64_t q, int32_t first_digit, int32_t behind) {
                if (is_match(c)) {
                    in_site = false;
                    if (!in_stretch) { in_stretch = true; stretch_from = q; }
                    stretch_to = q + len;
                    return;
                }
                close_stretch();
                if (!in_site) {
                    in_site = true;
                    of_row.push_back(Site{s + q, s + q, 0, 0, 0, first_digit, behind});
                }
                Site &k = of_row.back();
                (c == 'X' ? k.x : c == 'I' ? k.ins : k.del) += len;
                if (c != 'D') k.end += len;
                k.behind = behind;
            })))
            return rc;
        close_stretch();
        RibbitRowPurity &r = per_row[i];
        r = RibbitRowPurity{(int32_t)found.size(), (int32_t)of_row.size(), 0, 0, 0, (int32_t)query, (int32_t)(s + pure_from), (int32_t)(s + pure_to)};
        for (const Site &k : of_row) {
            found.push_back(RibbitInterruption{(int32_t)i, (int32_t)k.start, (int32_t)k.end, (int32_t)k.x, (int32_t)k.ins, (int32_t)k.del, k.at, k.behind - k.at});
            r.x += (int32_t)k.x;
            r.ins += (int32_t)k.ins;
            r.del += (int32_t)k.del;
            const int64_t a = std::min<int64_t>(std::max<int64_t>(k.start, 0), length), b = std::min<int64_t>(std::max<int64_t>(k.end, a), length);
            if ((int64_t)text.size() + (b - a) > (int64_t)INT32_MAX) return fail(RIBBIT_E_ARG, "the interruptions' observed bases are more than 2147483647 bytes");
            text.append(sequence + a, (size_t)(b - a));
            text_at.push_back((int32_t)text.size());
        }
    }
    Handed<RibbitRowPurity> out_rows;
    Handed<RibbitInterruption> out_sites;
    Handed<char> out_text;
    if ((rc = hand_out(per_row.data(), n, false, out_rows)) || (rc = hand_out(found.data(), found.size(), false, out_sites)) ||
        (rc = hand_out(text.data(), text.size(), true, out_text)) || (rc = hand_out(text_at.data(), text_at.size(), false, observed_offsets)))
        return rc;
    *rows = out_rows.release();
    *sites = out_sites.release();
    *n_sites = found.size();
    *observed = out_text.release();
    return RIBBIT_OK;
}

// ---- the CIGARs of a BED text: every row's last column
int bed_cigars_impl(const char *text, size_t len, char **pool, int32_t **offsets, size_t *n) {
    if (!pool || !offsets || !n || (!text && len > 0)) return fail(RIBBIT_E_ARG, "null argument");
    return bed_gather(text, len, "CIGARs", [](const BedRow &row) { return row.cigar; },
                      [](size_t at) { return fail(RIBBIT_E_ARG, "BED text at byte %zu is not a row of 11 tab-separated columns", at); }, pool, offsets, n);
}

// ---- the two outputs as text
inline bool consistent(const int32_t *intervals, const RibbitRowPurity *rows, size_t i) {
    return (int64_t)intervals[2 * i] + (int64_t)rows[i].query == (int64_t)intervals[2 * i + 1];
}

int interruption_text_impl(const char *name, const char *bed, size_t bed_len, const int32_t *intervals, size_t n, const RibbitRowPurity *rows,
                           const RibbitInterruption *sites, size_t n_sites, const char *cigars, const char *observed, const int32_t *observed_offsets, char **text,
                           size_t *len, size_t *rows_left_out) {
    if (!name || !text || !len || !rows_left_out || (!bed && bed_len > 0) || ((!intervals || !rows) && n > 0) || ((!sites || !observed_offsets) && n_sites > 0))
        return fail(RIBBIT_E_ARG, "null argument");
    if (n > MAX_ROWS || n_sites > MAX_ROWS) return fail(RIBBIT_E_ARG, "%zu rows with %zu interruptions", n, n_sites);
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    if (n_sites && observed_offsets[0] != 0) return fail(RIBBIT_E_ARG, "the observed bases' offsets start at %d, not at 0", (int)observed_offsets[0]);
    for (size_t j = 0; j < n_sites; ++j)
        if (observed_offsets[j + 1] < observed_offsets[j]) return fail(RIBBIT_E_ARG, "interruption %zu: the observed bases' offsets do not ascend", j);
    if (n_sites && observed_offsets[n_sites] > 0 && !observed) return fail(RIBBIT_E_ARG, "null argument");
    const size_t pool_len = cigars ? std::strlen(cigars) : 0, name_len = std::strlen(name);
    enum : int { FINE = 0, RANGE, OWNER, CIGAR, LINE };      // a refusal's why; a: the row, b: the interruption
    std::vector<size_t> left_out(parts, 0);
    rc = write_pieces(parts, "the interruptions", text, len, [&](size_t t, std::string &out) {
        for (size_t i = n * t / parts; i < n * (t + 1) / parts; ++i) {
            const RibbitRowPurity &r = rows[i];
            if (r.first < 0 || r.count < 0 || (size_t)r.first + (size_t)r.count > n_sites) return PieceRefusal{RANGE, i, 0};
            if (!consistent(intervals, rows, i)) { ++left_out[t]; continue; }
            if (r.count == 0) continue;
            const BedField line = lines[i];
            const BedField motif = bed_row(line.from, line.to).motif;      // (not a row: no motif)
            if (motif.to <= motif.from) return PieceRefusal{LINE, i, 0};
            const int64_t s = intervals[2 * i], k = (int64_t)motif.size();
            for (size_t j = (size_t)r.first; j < (size_t)r.first + (size_t)r.count; ++j) {
                const RibbitInterruption &site = sites[j];
                if (site.row < 0 || (size_t)site.row != i) return PieceRefusal{OWNER, i, j};
                if (site.cigar_at < 0 || site.cigar_len < 0 || (size_t)site.cigar_at + (size_t)site.cigar_len > pool_len) return PieceRefusal{CIGAR, i, j};
                out.append(name, name_len);
                out += '\t';
                put_number(out, site.start);
                out += '\t';
                put_number(out, site.end);
                out += '\t';
                out.append(cigars + site.cigar_at, (size_t)site.cigar_len);
                out += '\t';
                const int32_t from = observed_offsets[j], to = observed_offsets[j + 1];
                if (to > from) out.append(observed + from, (size_t)(to - from)); else out += '.';
                out += '\t';
                put_number(out, s);
                out += '\t';
                put_number(out, intervals[2 * i + 1]);
                out += '\t';
                put_field(out, motif);
                out += '\t';
                put_number(out, ((int64_t)site.start - s) / k);
                out += '\n';
            }
        }
        return PieceRefusal{};
    }, [&](const PieceRefusal &b) {
        switch (b.why) {
            case RANGE: return fail(RIBBIT_E_ARG, "row %zu: interruptions %d .. %lld of %zu", b.a, (int)rows[b.a].first, (long long)rows[b.a].first + rows[b.a].count, n_sites);
            case OWNER: return fail(RIBBIT_E_ARG, "row %zu: interruption %zu is row %d's", b.a, b.b, (int)sites[b.b].row);
            case CIGAR:
                return fail(RIBBIT_E_ARG, "interruption %zu: CIGAR bytes %d .. %lld of a pool of %zu", b.b, (int)sites[b.b].cigar_at,
                            (long long)sites[b.b].cigar_at + sites[b.b].cigar_len, pool_len);
            default: return fail(RIBBIT_E_ARG, "line %zu of the BED text is not a row of 11 tab-separated columns with a motif", b.a);
        }
    });
    if (rc) return rc;
    *rows_left_out = 0;
    for (const size_t l : left_out) *rows_left_out += l;
    return RIBBIT_OK;
}

int bed_purity_text_impl(const char *bed, size_t bed_len, const int32_t *intervals, const int32_t *motif_lengths, const RibbitRowPurity *rows, size_t n, char **text,
                         size_t *len) {
    if (!text || !len || (!bed && bed_len > 0) || ((!intervals || !motif_lengths || !rows) && n > 0)) return fail(RIBBIT_E_ARG, "null argument");
    const size_t parts = bed_text_parts(bed_len);
    BedLines lines;
    int rc;
    if ((rc = lines.find(bed, bed_len, parts))) return rc;
    if (lines.count() != n) return fail(RIBBIT_E_ARG, "the BED text has %zu lines, not the %zu of the rows", lines.count(), n);
    for (size_t i = 0; i < n; ++i)
        if (motif_lengths[i] < 1) return fail(RIBBIT_E_ARG, "row %zu: a motif of %d bases", i, (int)motif_lengths[i]);
    // piece k writes lines [n k / parts, n (k + 1) / parts): every line grows by seven columns
    return write_pieces(parts, "the rows' purity", text, len, [&](size_t k, std::string &out) {
        const size_t from = n * k / parts, to = n * (k + 1) / parts;
        out.reserve(lines.start[to] - lines.start[from] + 40 * (to - from));
        for (size_t i = from; i < to; ++i) {
            put_field(out, lines[i]);
            const RibbitRowPurity &r = rows[i];
            for (const int64_t v : {(int64_t)r.count, (int64_t)r.x, (int64_t)r.ins, (int64_t)r.del}) {
                out += '\t';
                put_number(out, v);
            }
            if (consistent(intervals, rows, i)) {
                for (const int64_t v : {(int64_t)r.pure_start, (int64_t)r.pure_end, ((int64_t)r.pure_end - (int64_t)r.pure_start) / (int64_t)motif_lengths[i]}) {
                    out += '\t';
                    put_number(out, v);
                }
            } else {
                out += "\t.\t.\t.";
            }
            out += '\n';
        }
    });
}

}  // namespace

extern "C" {

int ribbit_bed_cigars(const char *bed_text, size_t bed_len, char **pool, int32_t **offsets, size_t *n) {
    return guarded("reading the CIGARs", [&]() -> int { return bed_cigars_impl(bed_text, bed_len, pool, offsets, n); });
}

int ribbit_hip_record_interruptions(RibbitHandle *h, const int32_t *intervals, const int32_t *motif_lengths, size_t n, const char *cigars, const int32_t *offsets,
                                    const RibbitRowPurity **rows, const RibbitInterruption **sites, size_t *n_sites, const char **observed,
                                    const int32_t **observed_offsets) {
    return guarded("the interruptions", [&]() -> int {
        return record_interruptions_impl(h, intervals, motif_lengths, n, cigars, offsets, rows, sites, n_sites, observed, observed_offsets);
    });
}

int ribbit_host_record_interruptions(const char *sequence, int64_t length, const int32_t *intervals, const int32_t *motif_lengths, size_t n, const char *cigars,
                                     const int32_t *offsets, RibbitRowPurity **rows, RibbitInterruption **sites, size_t *n_sites, char **observed,
                                     int32_t **observed_offsets) {
    return guarded("the interruptions", [&]() -> int {
        return host_record_interruptions_impl(sequence, length, intervals, motif_lengths, n, cigars, offsets, rows, sites, n_sites, observed, observed_offsets);
    });
}

void ribbit_row_purity_free(RibbitRowPurity *rows) { std::free(rows); }
void ribbit_interruptions_free(RibbitInterruption *sites) { std::free(sites); }

int ribbit_interruption_text(const char *name, const char *bed_text, size_t bed_len, const int32_t *intervals, size_t n, const RibbitRowPurity *rows,
                             const RibbitInterruption *sites, size_t n_sites, const char *cigars, const char *observed, const int32_t *observed_offsets, char **text,
                             size_t *len, size_t *rows_left_out) {
    return guarded("the interruptions' text", [&]() -> int {
        return interruption_text_impl(name, bed_text, bed_len, intervals, n, rows, sites, n_sites, cigars, observed, observed_offsets, text, len, rows_left_out);
    });
}

int ribbit_bed_purity_text(const char *bed_text, size_t bed_len, const int32_t *intervals, const int32_t *motif_lengths, const RibbitRowPurity *rows, size_t n,
                           char **text, size_t *len) {
    return guarded("the rows' purity as text", [&]() -> int { return bed_purity_text_impl(bed_text, bed_len, intervals, motif_lengths, rows, n, text, len); });
}

}  // extern "C"
